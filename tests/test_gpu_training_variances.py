"""GPU: the HIP training step with phone-level and CWT variances (lightningfastspeech2_amd/training.py) against (a) the three
fixtures the REAL reference produced (tools/gen_golden_train_variances.py), (b) the CPU helper tests/_train_variances.py on
other shapes, and the two CWT-head operators (fs2_op_cwt_head_train / fs2_op_cwt_head_bwd) against float64 numpy.
Tolerances are those of tests/test_gpu_training.py: losses 1e-5 relative, gradients 1e-4 of the tensor's largest entry,
gradient norms 2e-4, learning rates 1e-12, weights after three steps 2e-5."""

import numpy as np
import pytest
import torch

from _train_variances import CASES, VarianceOracleTrainer, case, check_grads, load_fixture
from test_train_oracle import assert_params_close, load

pytestmark = pytest.mark.gpu
GRAD_TOL = 1e-4


def _dev(batch):
    return {k: torch.as_tensor(v).cuda() for k, v in batch.items()}


def _run_fixture(z, cfg, sd, batch, hyper):
    from lightningfastspeech2_amd.training import Trainer
    tr = Trainer(cfg, sd, **hyper)
    for step in (1, 2, 3):
        losses = tr.training_step(_dev(batch))
        if step == 1:
            assert list(losses) == [k[5:] for k in z.files if k.startswith("loss_")]
            for k, v in losses.items():
                w = float(z[f"loss_{k}"])
                print(f"loss {k}: {float(v):.8f} want {w:.8f}")
                assert abs(float(v) - w) <= 1e-5 * max(1.0, abs(w)), (k, float(v), w)
            check_grads(tr.gradients(), {k[5:]: z[k] for k in z.files if k.startswith("grad_")}, GRAD_TOL)
        norm = float(torch.sqrt((tr.flat_g.double() ** 2).sum()))
        assert abs(norm - float(z[f"gradnorm_{step}"])) <= 2e-4 * float(z[f"gradnorm_{step}"])
        lr = tr.optimizer_step()
        assert abs(lr - float(z[f"lr_{step}"])) <= 1e-12
    after = tr.state_dict()
    for k in z.files:
        if k.startswith("after3_"):
            assert_params_close(z, k[7:], after[k[7:]], 2e-5)
    return tr


@pytest.mark.parametrize("name", CASES)
def test_training_step_matches_reference_fixture(name):
    """1. losses (and their keys), gradients, gradient norms, learning rates and the weights after three steps"""
    z, cfg, sd, batch, hyper = load_fixture(name)
    tr = _run_fixture(z, cfg, sd, batch, hyper)
    for vi, v in enumerate(cfg.variances):
        got = tr.last[f"variances_{v}"]
        S = batch["phones"].shape[1] if cfg.is_phone_level(vi) else batch["mel"].shape[1]
        if cfg.is_cwt(vi):
            assert sorted(got) == ["mean", "spectrogram", "std"] and tuple(got["spectrogram"].shape) == (3, S, 10)
        else:
            assert tuple(got.shape) == (3, S)


DW = dict(encoder_depthwise_conv=True, decoder_depthwise_conv=True, variance_depthwise_conv=True, duration_depthwise_conv=True,
          encoder_conv_filter_size=128, decoder_conv_filter_size=192, decoder_kernel_sizes=[17, 3])
PRIORS = dict(priors=["pitch", "duration"], stats={"pitch_prior": {"min": -1.0, "max": 1.0}, "duration_prior": {"min": 0.0, "max": 5.0}})
CLASS_DEFAULT = (("phone", "phone", "phone"), ("cwt", "none", "none"))
SHAPES = [
    (3, 4, 13, [13, 9, 5, 1], *CLASS_DEFAULT, {}),                                                      # ragged, an utterance of one phone
    (5, 3, 21, [21, 8, 2], ("phone", "phone", "frame"), ("cwt", "none", "none"), DW),                   # depth-wise predictors
    (7, 3, 10, [10, 6, 8], ("phone", "frame"), ("cwt", "none"), PRIORS),                                # priors on
    (8, 2, 37, [37, 20], ("frame", "phone", "frame"), ("cwt", "none", "none"), {}),                     # exactly one phone-level variance
]


@pytest.mark.parametrize("seed,B,L,lengths,levels,transforms,kw", SHAPES)
def test_training_step_matches_cpu_helper_on_other_shapes(seed, B, L, lengths, levels, transforms, kw):
    """2. variance_losses mix l1 and mse, with l1 on the CWT spectrogram"""
    from lightningfastspeech2_amd.training import Trainer
    cfg, sd, batch = case(seed, B, L, lengths, levels, transforms, **kw)
    hyper = dict(lr=1e-3, warmup_steps=2, gradient_clip_val=0.5, variance_losses=["l1", "mse", "l1"][:len(levels)], mel_loss="mse",
                 duration_loss="l1")
    ref = VarianceOracleTrainer(cfg, sd, **hyper)
    want_l, _ = ref.training_step(batch)
    tr = Trainer(cfg, sd, **hyper)
    got_l = tr.training_step(_dev(batch))
    assert list(got_l) == list(want_l)
    for k, w in want_l.items():
        assert abs(float(got_l[k]) - w) <= 1e-5 * max(1.0, abs(w)), (k, float(got_l[k]), w)
    check_grads(tr.gradients(), ref.gradients(), GRAD_TOL)


def test_gradient_accumulation_and_bit_equal_reruns():
    """3. two micro-batches accumulate; the same step from the same state gives bit-equal flat gradients"""
    from lightningfastspeech2_amd.training import Trainer
    cfg, sd, b1 = case(21, 3, 11, [11, 6, 2], *CLASS_DEFAULT)
    _, _, b2 = case(22, 3, 11, [11, 10, 7], *CLASS_DEFAULT)
    kw = dict(lr=1e-3, warmup_steps=2, gradient_clip_val=1.0)
    ref = VarianceOracleTrainer(cfg, sd, **kw)
    ref.training_step(b1)
    ref.training_step(b2)
    tr = Trainer(cfg, sd, **kw)
    tr.training_step(_dev(b1))
    g1 = tr.flat_g.clone()
    tr.training_step(_dev(b2))
    check_grads(tr.gradients(), ref.gradients(), GRAD_TOL)
    tr2 = Trainer(cfg, sd, **kw)
    tr2.training_step(_dev(b1))
    assert torch.equal(tr2.flat_g, g1)
    tr2.training_step(_dev(b2))
    assert torch.equal(tr2.flat_g, tr.flat_g)


def test_backward_is_the_derivative_of_the_forward_under_dropout():
    """4. the reference's dropout defaults (0.1 encoder / 0.1 decoder / 0.5 predictors) on the class-default fixture's configuration:
    the method and tolerance of test_gpu_training.test_backward_is_the_derivative_of_the_forward_under_dropout"""
    from lightningfastspeech2_amd.training import Trainer
    _, cfg, sd, batch, _ = load_fixture("train_classdefault_small")
    drop = dict(encoder_dropout=0.1, decoder_dropout=0.1, variance_dropout=0.5, duration_dropout=0.5, seed=9)
    tr = Trainer(cfg, sd, gradient_clip_val=None, **drop)
    bd = _dev(batch)
    l0 = tr.training_step(bd)
    g = tr.flat_g.clone().double()
    tr.zero_grad()
    tr._micro = 0
    again = tr.training_step(bd)  # same seed, same masks: the same losses
    assert all(float(again[k]) == float(l0[k]) for k in l0)
    tr.zero_grad()
    tr0 = Trainer(cfg, sd, gradient_clip_val=None)
    assert abs(float(tr0.training_step(bd)["total"]) - float(l0["total"])) > 1e-3  # dropout really is on
    w0 = tr.flat_p.clone()
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    for trial in range(3):
        v = g.float() * (0.5 + torch.rand(tr.n_flat, device="cuda:0", generator=gen))
        eps = 1e-4 / float(v.norm()) * float(w0.norm())
        vals = []
        for sgn in (1.0, -1.0):
            tr.flat_p.copy_(w0 + sgn * eps * v)
            tr._refresh_shadow()
            tr._micro = 0
            vals.append(float(tr.training_step(bd)["total"].double()))
            tr.zero_grad()
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = float((g * v.double()).sum())
        print(f"trial {trial}: finite difference {fd:.6f} analytic {an:.6f}")
        assert an > 0 and abs(fd - an) <= 3e-2 * an, (trial, fd, an)


def test_bf16_mixed_precision_step_tracks_the_fp32_gradients():
    """5. the criteria of test_gpu_training's bf16 test on the class-default configuration"""
    from lightningfastspeech2_amd.training import Trainer
    _, cfg, sd, batch, hyper = load_fixture("train_classdefault_small")
    ref = VarianceOracleTrainer(cfg, sd, **hyper)
    want_l, _ = ref.training_step(batch)
    want = ref.gradients()
    tr = Trainer(cfg, sd, precision="bf16", **hyper)
    got_l = tr.training_step(_dev(batch))
    for k, w in want_l.items():
        assert abs(float(got_l[k]) - w) <= 2e-2 * max(1.0, abs(w)), (k, float(got_l[k]), w)
    got = tr.gradients()
    worst = ("", 1.0)
    gmax = max(float(w.abs().max()) for w in want.values())
    for n, w in want.items():
        if float(w.abs().max()) < 1e-4 * gmax:
            continue
        cos = float((got[n].double() * w.double()).sum() / (got[n].double().norm() * w.double().norm() + 1e-30))
        if cos < worst[1]:
            worst = (n, cos)
    assert worst[1] >= 0.99, worst
    first = float(got_l["total"])
    tr.optimizer_step()
    for _ in range(3):
        last = float(tr.training_step(_dev(batch))["total"])
        tr.optimizer_step()
    assert last < first


# ---- 6. the two operators ----
def _op_inputs(B, S, F, tdt, seed):
    rs = np.random.RandomState(seed)
    y = torch.from_numpy(rs.randn(B * S, F).astype(np.float32)).to(tdt)
    # the first utterance has a single valid row, the last one no pads
    lengths = [S] if B == 1 else [1] + [int(rs.randint(1, S + 1)) for _ in range(B - 2)] + [S]
    mask = np.ones((B, S), dtype=np.uint8)
    for b, n in enumerate(lengths):
        mask[b, :n] = 0
    f = lambda *s: rs.randn(*s).astype(np.float32)
    sc = np.float32(1.0 / np.sqrt(F))  # a float32 scalar: a float64 one would promote the weights, which the kernels read as fp32
    d = dict(y=y, mask=mask, w10=f(10, F) * sc, b10=f(10), ms_w=f(2, F) * sc, ms_b=f(2), dspec=f(B * S, 10) * (1 - mask.reshape(-1, 1)),
             dms=f(B, 2), g_w10=f(10, F), g_b10=f(10), g_ms_w=f(2, F), g_ms_b=f(2))
    assert all(v.dtype == np.float32 for k, v in d.items() if k not in ("y", "mask"))
    return d


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got.double().cpu().numpy() - want).max()
    assert err <= 1e-4 * np.abs(want).max(), (what, err, np.abs(want).max())


@pytest.mark.parametrize("B,S,F", [(1, 1, 64), (3, 37, 64), (2, 257, 256), (2, 70, 768)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_cwt_head_operators_match_float64(B, S, F, dtype):
    from lightningfastspeech2_amd import _lib
    lib = _lib.load()
    dt, tdt = (_lib.FS2_F32, torch.float32) if dtype == "fp32" else (_lib.FS2_BF16, torch.bfloat16)
    d = _op_inputs(B, S, F, tdt, 100 + S)
    st = torch.cuda.current_stream()
    dev = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).cuda() for k, v in d.items()}
    y64 = d["y"].double().numpy()
    valid = 1.0 - d["mask"].reshape(-1, 1).astype(np.float64)
    spec_w = (y64 @ d["w10"].astype(np.float64).T + d["b10"]) * valid
    ybar_w = y64.reshape(B, S, F).mean(1)
    ms_w_ = ybar_w @ d["ms_w"].astype(np.float64).T + d["ms_b"]
    runs = []
    for _ in range(2):
        spec, ybar, ms = (torch.full((B * S, 10), 7.0, device="cuda"), torch.full((B, F), 7.0, device="cuda"), torch.full((B, 2), 7.0, device="cuda"))
        ws = torch.zeros(int(lib.fs2_op_cwt_head_train_ws_bytes(B, S, F)) // 4 + 1, device="cuda")
        _lib.check(lib.fs2_op_cwt_head_train(dt, dev["y"], dev["w10"], dev["b10"], dev["ms_w"], dev["ms_b"], dev["mask"], spec, ybar, ms,
                                             ws, B, S, F, st))
        runs.append((spec, ybar, ms))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    _close(runs[0][0], spec_w, "spec")
    _close(runs[0][1], ybar_w, "ybar")
    _close(runs[0][2], ms_w_, "mean_std")
    # backward: ybar as the forward's (rounded to fp32); g_* are ADDED to non-zero contents
    ybar32 = torch.from_numpy(ybar_w.astype(np.float32)).cuda()
    ds64, dms64 = d["dspec"].astype(np.float64), d["dms"].astype(np.float64)
    dy_w = ds64 @ d["w10"].astype(np.float64) + np.repeat(dms64 @ d["ms_w"].astype(np.float64), S, axis=0) / S
    want = dict(g_w10=d["g_w10"] + ds64.T @ y64, g_b10=d["g_b10"] + ds64.sum(0),
                g_ms_w=d["g_ms_w"] + dms64.T @ ybar32.double().cpu().numpy(), g_ms_b=d["g_ms_b"] + dms64.sum(0))
    runs = []
    for _ in range(2):
        g = {k: dev[k].clone() for k in want}
        dy = torch.full((B * S, F), 7.0, device="cuda", dtype=tdt)
        ws = torch.zeros(int(lib.fs2_op_cwt_head_bwd_ws_bytes(B, S, F)) // 4 + 1, device="cuda")
        _lib.check(lib.fs2_op_cwt_head_bwd(dt, dev["y"], dev["dspec"], dev["dms"], ybar32, dev["w10"], dev["ms_w"], dy, g["g_w10"],
                                           g["g_b10"], g["g_ms_w"], g["g_ms_b"], ws, B, S, F, st))
        runs.append((dy, g))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in want:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
        _close(runs[0][1][k], want[k], k)
    dy = runs[0][0].double().cpu().numpy()
    if dtype == "fp32":
        _close(runs[0][0], dy_w, "dy")
    else:  # one output rounding + fp32 accumulation
        assert (np.abs(dy - dy_w) <= 2.0 ** -8 * np.abs(dy_w) + 1e-4 * np.abs(dy_w).max()).all()
    pad = d["mask"].reshape(-1).astype(bool)
    if pad.any():  # a pad row still receives the mean / std term
        assert np.abs(dy[pad]).max() > 0


def test_cwt_head_operators_reject_an_unsupported_width():
    from lightningfastspeech2_amd import _lib
    lib = _lib.load()
    B, S, F = 2, 5, 100
    st = torch.cuda.current_stream()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, device="cuda", dtype=dtype)
    y, w10, b10, msw, msb, mask = z(B * S, 128), z(10, 128), z(10), z(2, 128), z(2), z(B * S, dtype=torch.uint8)
    spec, ybar, ms, ws, dy = z(B * S, 10), z(B, 128), z(B, 2), z(1 << 16), z(B * S, 128)
    for F_ in (F, 32, 1088):
        assert lib.fs2_op_cwt_head_train(_lib.FS2_F32, y, w10, b10, msw, msb, mask, spec, ybar, ms, ws, B, S, F_, st) == _lib.FS2_ERR_ARG
        assert lib.fs2_op_cwt_head_bwd(_lib.FS2_F32, y, spec, ms, ybar, w10, msw, dy, w10.clone(), b10, msw.clone(), msb, ws, B, S, F_, st) == _lib.FS2_ERR_ARG
    torch.cuda.synchronize()


def test_all_frame_configuration_is_unchanged():
    """7. an all-frame, all-'none' configuration: the untouched train_small.npz through the machinery of test 1, and two Trainers
    give bit-equal flat gradients"""
    from lightningfastspeech2_amd.training import Trainer
    z, cfg, sd, batch, hyper = load("train_small")
    _run_fixture(z, cfg, sd, batch, hyper)
    a, b = Trainer(cfg, sd, **hyper), Trainer(cfg, sd, **hyper)
    a.training_step(_dev(batch))
    b.training_step(_dev(batch))
    assert torch.equal(a.flat_g, b.flat_g)


def test_argument_checks():
    """8."""
    from lightningfastspeech2_amd.training import Trainer
    _, cfg, sd, batch, hyper = load_fixture("train_classdefault_small")
    tr = Trainer(cfg, sd, **hyper)
    B, T = batch["mel"].shape[:2]
    bad = dict(batch, variances_energy=np.zeros((B, T), dtype=np.float32))  # phone-level energy takes (B, L)
    with pytest.raises(ValueError, match="variances_energy"):
        tr.training_step(_dev(bad))
    with pytest.raises(ValueError, match="variances_pitch_spectrogram"):
        tr.training_step(_dev({k: v for k, v in batch.items() if k != "variances_pitch_spectrogram"}))
    _, pcfg, psd, pbatch, phyper = load_fixture("train_phone_small")
    with pytest.raises(ValueError, match="variances_pitch"):
        Trainer(pcfg, psd, **phyper).training_step(_dev(dict(pbatch, variances_pitch=np.zeros((B, pbatch["mel"].shape[1]), dtype=np.float32))))
    with pytest.raises(NotImplementedError, match="soft_dtw"):
        Trainer(cfg, sd, variance_losses=["soft_dtw", "mse", "mse"])
