"""The restatement of the training attention (tests/_attn_train_ref.py) checked on the CPU before tests/test_gpu_attention_train.py
relies on it: the float64 closed form against float64 autograd, the judging rules against restatements damaged on purpose, and the
yardsticks (the float32 and the storage-rounded restatement's own errors) of every shape the GPU file runs, printed (pytest -s)."""
import pytest
import torch

import _attn_train_ref as R


def keep_mask(B, S, heads, p, seed):
    return torch.rand(B, heads, S, S, generator=torch.Generator().manual_seed(seed)) >= p


def case(B, S, heads, kind="suffix", seed=0):
    qkv, dout = R.inputs(B, S, heads, seed or (S + heads))
    return qkv, R.mask_of(kind, B, S), dout


def seam_case(S, heads=2):
    lens = R.seam_lengths(S)
    B = len(lens)
    qkv, dout = R.inputs(B, S, heads, 1000 + S)
    return qkv, torch.arange(S)[None, :] >= torch.tensor(lens)[:, None], dout, B


@pytest.mark.parametrize("B,S,heads,kind,p", [(2, 37, 2, "suffix", 0.0), (2, 70, 2, "scatter", 0.2), (3, 65, 1, "holes", 0.0),
                                             (1, 1, 1, "none", 0.0), (2, 130, 2, "prefix", 0.3)])
def test_closed_form_equals_float64_autograd(B, S, heads, kind, p):
    qkv, pad, dout = case(B, S, heads, kind)
    keep = keep_mask(B, S, heads, p, 3) if p > 0 else None
    got = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "f64")
    want = R.autograd_truth(qkv, pad, dout, B, S, heads, keep, p)
    for name in ("out", "lse2", "dq", "dk", "dv"):
        scale = float(want[name].abs().max()) or 1.0
        err = float((got[name] - want[name]).abs().max())
        assert err <= 1e-12 * scale, (name, err, scale)
    # delta = sum_d dO out = sum_k P dP, and lse2 normalises the backward's P
    s2 = R.scores2(qkv, pad, B, S, heads)
    assert float((torch.exp2(s2 - got["lse2"][..., None]).sum(-1) - 1).abs().max()) <= 1e-12
    assert torch.equal(got["delta"], R.delta_of(dout, got["out"], B, S, heads))


def test_bf16_round_is_nearest_even_and_trunc_chops():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, 3.14159, 1e-3, 6e4], dtype=torch.float64)
    assert torch.equal(R.bf16_round(x).float(), x.float().to(torch.bfloat16).float())   # ties to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert torch.equal(R.bf16_trunc(x)[:3], torch.tensor([1.0, 1.0, 1.0078125], dtype=torch.float64))
    y = torch.randn(4096, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert torch.equal(R.bf16_round(y).float(), y.float().to(torch.bfloat16).float())


@pytest.mark.parametrize("S,p", [(65, 0.0), (129, 0.2)])
def test_rules_can_fail(S, p):
    """The honest bf16 restatement meets the 2 x rule against itself with ratio 1; a truncating one, one without a 16-key block of
    dQ and one with one row's lse2 off by 2^-6 do not."""
    qkv, pad, dout, B = seam_case(S)
    heads = 2
    keep = keep_mask(B, S, heads, p, 5) if p > 0 else None
    truth = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "f64")
    f32 = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "f32")
    model = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "bf16")
    floor = R.grad_floor(qkv, dout, B, S, heads)
    for name in ("out", "dq", "dk", "dv"):
        ok, fig = R.ratio_2x(model[name], truth[name], model[name], floor if name != "out" else 0.0)
        assert ok and fig["ratio_max"] == 1.0 and fig["ratio_rms"] == 1.0, (name, fig)
        print(f"{name}: fp32 floor {floor:.2e} against 2 x {fig['ref_max']:.2e}")
        assert name == "out" or floor <= 0.02 * 2 * fig["ref_max"]   # the fp32 floor is no real part of these bounds
    for name in ("lse2", "delta"):                          # the f32 restatement is within MARGIN of itself
        assert R.errs(f32[name], truth[name])[0] <= R.fp32_bound(f32[name], truth[name])
    # (i) truncation in place of rounding (ratios 2.5 .. 2.8 without dropout; with it out and dv at 3.5 / 4.3, dq at 1.84 / 1.87: the
    # rule fails on out and dv either way)
    trunc = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "bf16", rnd=R.bf16_trunc)
    failed = []
    for name in ("out", "dq", "dk", "dv"):
        ok, fig = R.ratio_2x(trunc[name], truth[name], model[name], floor if name != "out" else 0.0)
        print(f"truncated {name}: ratio {fig['ratio_max']:.2f} / {fig['ratio_rms']:.2f}")
        failed = failed + [name] * (not ok)
    assert "out" in failed and "dv" in failed, failed
    # (ii) one 16-key block missing from dQ of (utterance 0, head 1)
    hole = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "bf16", damage={"dq_block": (0, 1, 16)})
    ok, fig = R.ratio_2x(hole["dq"], truth["dq"], model["dq"], floor)
    print(f"dQ without keys 16..31: ratio {fig['ratio_max']:.2f} / {fig['ratio_rms']:.2f}")
    assert not ok
    for name in ("dk", "dv"):
        assert torch.equal(hole[name], model[name])
    # (iii) one row's lse2 + 2^-6: the fp32 rule on lse2 fails by orders of magnitude, and the 2 x rule on that utterance's gradients
    # fails too (every probability of the row is off by 1.1 %, three bf16 roundings' worth)
    row = int(truth["dq"][:S, 128:256].abs().max(dim=1).values.argmax())
    bad = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "bf16", damage={"lse_row": (0, 1, row, 2.0 ** -6)})
    assert R.errs(model["lse2"], truth["lse2"])[0] <= R.fp32_bound(f32["lse2"], truth["lse2"])
    assert R.errs(bad["lse2"], truth["lse2"])[0] > 100 * R.fp32_bound(f32["lse2"], truth["lse2"])
    sl = (slice(row, row + 1), slice(128, 256))
    ok, fig = R.ratio_2x(bad["dq"][sl], truth["dq"][sl], model["dq"][sl], floor)
    print(f"dQ of the row whose lse2 moved: ratio {fig['ratio_max']:.2f} / {fig['ratio_rms']:.2f}")
    assert not ok


def yardsticks(what, qkv, pad, dout, B, S, heads, keep=None, p=0.0):
    truth = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "f64")
    f32 = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "f32")
    model = R.attention_train(qkv, pad, dout, B, S, heads, keep, p, "bf16")
    y = {n: R.errs(f32[n], truth[n])[0] for n in ("lse2", "delta")}
    line = (f"{what}: f32 lse2 {y['lse2']:.2e} delta {y['delta']:.2e} (2^-23 max|lse2| {R.EPS32 * float(truth['lse2'].abs().max()):.2e});"
            f" bf16 max / rms")
    for n in ("out", "dq", "dk", "dv"):
        e = R.errs(model[n], truth[n])
        line += f" {n} {e[0]:.2e} / {e[1]:.2e}"
        ok, _ = R.ratio_2x(model[n], truth[n], model[n])
        assert ok
    for n in ("lse2", "delta"):
        assert y[n] <= R.fp32_bound(f32[n], truth[n])
    assert torch.isfinite(torch.cat([model[n].reshape(-1) for n in model])).all()
    print(line)


def test_yardsticks_of_every_gpu_shape():
    """what the GPU file's device errors are to be compared with; the reference alone meets every rule on every shape"""
    for B, S, heads, kind in R.FORWARD_CASES:
        yardsticks(f"forward ({B}, {S}, {heads}, {kind})", *case(B, S, heads, kind), B, S, heads)
    for pair in R.BYSIZE_CASES:
        for B, S, heads in pair:
            qkv, pad, dout = case(B, S, heads, "suffix")
            yardsticks(f"by size ({B}, {S}, {heads})", qkv, pad, dout, B, S, heads)
    for S in R.SEAM_S:
        qkv, pad, dout, B = seam_case(S)
        for p in (0.0, 0.2):
            keep = keep_mask(B, S, 2, p, S) if p > 0 else None
            yardsticks(f"seam S {S} drop {p}", qkv, pad, dout, B, S, 2, keep, p)
    qkv, dout = R.inputs(32, 20, 16, 3220)
    yardsticks("route (32, 20, 16)", qkv, torch.zeros(32, 20, dtype=torch.bool), dout, 32, 20, 16)
    for name, (qkv, pad, (B, S, heads), rows) in (("far rows", R.far_rows_qkv()), ("spike", R.spike_qkv())):
        dout = R.inputs(B, S, heads, 77)[1]
        yardsticks(f"rerun {name}", qkv, pad, dout, B, S, heads)
