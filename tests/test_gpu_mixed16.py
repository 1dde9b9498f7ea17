"""End-to-end tests of precision="mixed16" (FS2_MIXED_F16_X3; `-m gpu`): the front is "mixed3"'s bit for bit, the decoder is held to
a CPU model of a 16-bit-storage decoder (tests/_f16.py: decoder_16bit - the yardstick is that model, never the kernels' own output),
saturation inside the forward, the goldens' decisions, the plumbing (repeatability, pipeline, graphs, shards, shapes) and the
dispatch switches.  The four architectures are tests/test_gpu_forward.py's CASES, restated (same configs, B, L, lengths,
duration_bias, seed 3).  Measured values go to the parity report the other end-to-end tests write (test_gpu_forward._report)."""
import functools
import json

import numpy as np
import pytest
import torch

import _f16
from _golden import Golden, golden_names
from test_gpu_forward import _report
from lightningfastspeech2_amd.config import Fs2Config, preset
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
from oracle import oracle_cpu

pytestmark = pytest.mark.gpu

SEED = 3
CASES = {
    "c2arch_ragged": (lambda: preset("c2"), 4, 64, [64, 50, 33, 7], dict(duration_bias=1.5)),
    "refdefault_dw": (lambda: preset("ref-default"), 3, 48, [48, 30, 11], dict(duration_bias=1.4)),
    "ls_h768_2layer": (lambda: Fs2Config(**{**preset("c3").to_dict(), "encoder_layers": 1, "decoder_layers": 2,
                                            "variance_nlayers": [2, 2, 2]}), 2, 40, [40, 22], dict(duration_bias=1.3)),
    "h1024_dense_1layer": (lambda: Fs2Config(**{**preset("c5").to_dict(), "encoder_layers": 1, "decoder_layers": 1,
                                                "variance_nlayers": [1, 1, 1], "duration_nlayers": 1}),
                           2, 24, [24, 9], dict(duration_bias=1.3)),
}


def _model(cfg, sd, precision):
    from lightningfastspeech2_amd.model import FastSpeech2
    return FastSpeech2(cfg, sd, precision=precision, device="cuda:0")


def _cpu(d):
    return {k: ({kk: vv.cpu() for kk, vv in v.items()} if isinstance(v, dict) else v.cpu()) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case(case):
    """One oracle run per architecture, shared (and left unchanged) by every test that needs it."""
    mk, B, L, lengths, skw = CASES[case]
    cfg = mk()
    sd = synth_state_dict(cfg, SEED, randomize_norm=True, **skw)
    inp = synth_inputs(cfg, B, L, seed=SEED + 50, lengths=lengths)
    ref = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"], return_intermediates=True)
    batch = {"phones": torch.from_numpy(inp["phones"]), "speaker": torch.from_numpy(inp["speaker"])}
    forced = dict(force_durations=ref["duration_rounded"], force_buckets={v: ref["_intermediates"][f"bucket_{v}"] for v in cfg.variances})
    return cfg, sd, inp, ref, batch, forced


@functools.lru_cache(maxsize=None)
def _yardstick(case, tdt):
    """(max, mean) |mel - oracle| of the CPU model of a decoder storing in `tdt`, on the oracle's adaptor output."""
    cfg, sd, inp, ref, _, _ = _case(case)
    mel = _f16.decoder_16bit(sd, cfg, ref["_intermediates"]["adaptor_out"], inp["speaker"], ref["tgt_mask"], tdt)
    e = (mel - ref["mel"]).abs()
    return float(e.max()), float(e.mean()), mel


def _same(a, b, what):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), (what, k)
        elif isinstance(a[k], dict):
            for kk in a[k]:
                assert torch.equal(a[k][kk], b[k][kk]), (what, k, kk)


# ---- 1. the front ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_front_is_mixed3_bit_for_bit(case):
    """Free-running: every decision, prediction and front-side tensor of "mixed16" equals "mixed3"'s exactly - with the launches
    the served path takes (embedding tails fused into the predictor launches) and with the debug taps on (unfused)."""
    cfg, sd, _, _, batch, _ = _case(case)
    m16, m3 = _model(cfg, sd, "mixed16"), _model(cfg, sd, "mixed3")
    keys = ["duration_prediction", "duration_rounded", "src_mask", "tgt_mask"] + [f"variances_{v}" for v in cfg.variances]
    for debug in (False, True):
        m16.engine.set_debug(debug)
        m3.engine.set_debug(debug)
        a, b = _cpu(m16(batch, inference=True)), _cpu(m3(batch, inference=True))
        for k in keys:
            assert torch.equal(a[k], b[k]), (case, debug, k)
        assert a["mel"].shape == b["mel"].shape and not torch.equal(a["mel"], b["mel"])   # (another decoder did run)
    for tap in ["encoder_out", "adaptor_out"] + [f"bucket_{v}" for v in cfg.variances]:
        assert torch.equal(m16.engine.debug_tensor(tap).cpu(), m3.engine.debug_tensor(tap).cpu()), (case, tap)


# ---- 2. the decoder against the CPU model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_decoder_against_the_16bit_storage_model(case):
    """Durations and buckets forced to the oracle's.  (a) the model is calibrated: "mixed3"'s error lies within [1/2, 2] x the model's
    bf16 figures; (b) "mixed16" <= 2 x the model's fp16 figures (the factor (a) allows: summation order, folded weights); (c)
    "mixed16" <= "mixed3" / 4 (unit-roundoff ratio 8, a factor 2 left); (d) finite everywhere, pad rows included.

    Measured (max / mean |mel - oracle|: model bf16, mixed3, model fp16, mixed16):
    c2arch_ragged 1.65e-2 / 2.57e-3, 1.64e-2 / 2.58e-3, 1.82e-3 / 3.20e-4, 1.80e-3 / 3.22e-4; refdefault_dw 1.32e-2 / 2.36e-3,
    1.24e-2 / 2.36e-3, 1.57e-3 / 2.96e-4, 1.68e-3 / 2.99e-4; ls_h768_2layer 1.05e-2 / 1.97e-3, 9.42e-3 / 1.96e-3, 1.17e-3 / 2.42e-4,
    1.24e-3 / 2.46e-4; h1024_dense_1layer 8.12e-3 / 1.64e-3, 7.77e-3 / 1.68e-3, 9.39e-4 / 2.05e-4, 1.09e-3 / 2.11e-4."""
    cfg, sd, _, ref, batch, forced = _case(case)
    yb_max, yb_mean, _ = _yardstick(case, torch.bfloat16)
    yh_max, yh_mean, _ = _yardstick(case, torch.float16)
    e3 = (_cpu(_model(cfg, sd, "mixed3").forward(batch, **forced))["mel"] - ref["mel"]).abs()
    out16 = _cpu(_model(cfg, sd, "mixed16").forward(batch, **forced))
    e16 = (out16["mel"] - ref["mel"]).abs()
    m3_max, m3_mean, m16_max, m16_mean = float(e3.max()), float(e3.mean()), float(e16.max()), float(e16.mean())
    rec = dict(test="mixed16_decoder", case=case, mel_scale=float(ref["mel"].abs().max()), model_bf16=[yb_max, yb_mean], mixed3=[m3_max, m3_mean],
               model_fp16=[yh_max, yh_mean], mixed16=[m16_max, m16_mean], ratio_mixed3_over_mixed16=[m3_max / m16_max, m3_mean / m16_mean])
    _report(**rec)
    print(json.dumps(rec))
    assert bool(torch.isfinite(out16["mel"]).all())                                        # (d)
    assert torch.equal(out16["tgt_mask"], ref["tgt_mask"])
    assert 0.5 * yb_max <= m3_max <= 2 * yb_max and 0.5 * yb_mean <= m3_mean <= 2 * yb_mean, rec   # (a)
    assert m16_max <= 2 * yh_max and m16_mean <= 2 * yh_mean, rec                           # (b)
    assert m16_max <= m3_max / 4 and m16_mean <= m3_mean / 4, rec                           # (c)


# ---- 3. goldens --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in golden_names() if "teacher" not in n])
def test_decisions_on_goldens(name):
    g = Golden(name)
    batch = {"phones": torch.from_numpy(g.phones), "speaker": torch.from_numpy(g.speaker), **g.priors}
    out = _cpu(_model(g.cfg, g.state_dict(), "mixed16")(batch, inference=True))
    for k in ("duration_rounded", "src_mask", "tgt_mask"):
        assert np.array_equal(out[k].numpy(), g.out[k]), k
    out3 = _cpu(_model(g.cfg, g.state_dict(), "mixed3")(batch, inference=True))
    err, err3 = float(np.abs(out["mel"].numpy() - g.out["mel"]).max()), float(np.abs(out3["mel"].numpy() - g.out["mel"]).max())
    _report(test="golden_mixed16", case=name, mel_max=err, mel_max_mixed3=err3, mel_scale=float(np.abs(g.out["mel"]).max()))
    assert np.isfinite(err) and err < err3, (err, err3)


# ---- 4. saturation inside the forward ----------------------------------------------------------------------------------------------
def test_ffn_overflow_saturates_and_stays_finite():
    """The last decoder block's conv1 bias raised to +1e5 on 8 channels: the post-ReLU FFN tensor exceeds 65504 there on every frame.
    The stores clamp (no infinity reaches conv2, no NaN leaves the LayerNorm behind it): the mel is finite, equals the CPU
    model's with the same clamp within the bound of test 2 (b), and is not the unmodified run's."""
    case = "c2arch_ragged"
    cfg, sd, inp, ref, batch, forced = _case(case)
    yh_max, yh_mean, _ = _yardstick(case, torch.float16)
    name = f"decoder.layers.{cfg.decoder_layers - 1}.conv1.bias"
    sd2 = dict(sd)
    bias = np.array(sd[name], dtype=np.float32, copy=True)
    bias[3:3 + 8 * 37:37] = 1e5
    sd2[name] = bias
    want = _f16.decoder_16bit(sd2, cfg, ref["_intermediates"]["adaptor_out"], inp["speaker"], ref["tgt_mask"], torch.float16)
    assert bool(torch.isfinite(want).all())
    got = _cpu(_model(cfg, sd2, "mixed16").forward(batch, **forced))["mel"]
    plain = _cpu(_model(cfg, sd, "mixed16").forward(batch, **forced))["mel"]
    assert bool(torch.isfinite(got).all())
    e = (got - want).abs()
    _report(test="mixed16_saturation", case=case, vs_model=[float(e.max()), float(e.mean())], bound=[2 * yh_max, 2 * yh_mean],
            moved=float((got - plain).abs().max()))
    assert float(e.max()) <= 2 * yh_max and float(e.mean()) <= 2 * yh_mean, (float(e.max()), float(e.mean()), yh_max, yh_mean)
    assert float((got - plain).abs().max()) > 100 * yh_max   # the clamp path was taken: another mel altogether


# ---- 5. plumbing -------------------------------------------------------------------------------------------------------------------
def test_plumbing_repeat_pipeline_graphs_shards_shapes():
    cfg, sd, inp, ref, batch, _ = _case("refdefault_dw")
    m = _model(cfg, sd, "mixed16")
    dev = {k: v.to("cuda:0") for k, v in batch.items()}
    first = _cpu(m(dev, inference=True))
    _same(first, _cpu(m(dev, inference=True)), "second call")
    # pipeline(2) over 4 batches, in submission order, against serial calls
    batches = []
    for s in range(4):
        i2 = synth_inputs(cfg, 3, 48, seed=200 + s, lengths=[48, 30 - s, 11 + s])
        batches.append({"phones": torch.from_numpy(i2["phones"]).to("cuda:0"), "speaker": torch.from_numpy(i2["speaker"]).to("cuda:0")})
    serial = [_cpu(m(b, inference=True)) for b in batches]
    pipe = m.pipeline(2)
    try:
        got = []
        for b in batches:
            got += [_cpu(o) for o in pipe.submit(b)]
        got += [_cpu(o) for o in pipe.drain()]
    finally:
        pipe.close()
    assert len(got) == 4
    for i, (a, b) in enumerate(zip(got, serial)):
        _same(a, b, f"pipeline result {i}")
    # a batch in two shards, padded to the whole batch's frame count: the rows of the whole
    T = first["mel"].shape[1]
    for lo, hi in ((0, 2), (2, 3)):
        sh = {k: v[lo:hi].contiguous() for k, v in dev.items()}
        part = _cpu(m.forward(sh, inference=True, frames_hook=lambda t: T))
        for k in ("mel", "tgt_mask", "duration_rounded", "duration_prediction"):
            assert torch.equal(part[k], first[k][lo:hi]), ("shard", lo, k)
    # another shape through the same model, then the first one again
    i3 = synth_inputs(cfg, 2, 33, seed=300, lengths=[33, 20])
    other = _cpu(m({"phones": torch.from_numpy(i3["phones"]), "speaker": torch.from_numpy(i3["speaker"])}, inference=True))
    assert other["mel"].shape[0] == 2 and bool(torch.isfinite(other["mel"]).all())
    _same(first, _cpu(m(dev, inference=True)), "after another shape")
    # graph replay against eager
    g = _model(cfg, sd, "mixed16")
    g.engine.set_graphs(True)
    n0 = g.engine.graph_replays()
    outs = [_cpu(g(dev, inference=True)) for _ in range(4)]
    assert g.engine.graph_replays() > n0, "no phase was replayed as a graph"
    for i, o in enumerate(outs):
        _same(o, first, f"graphs call {i}")


# ---- 6. dispatch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["c2arch_ragged", "ls_h768_2layer"])
def test_dispatch_switches_leave_the_bits(case):
    """The weight-resident GEMM (1402: wherever it applies / 1400: never) is bit-identical to the slab kernel: so is the
    forced-decision mel with it switched - on c2arch_ragged, whose K = 256 GEMMs it takes when forced; at these sizes (a few hundred
    rows) the default never picks it, and the persistent GEMM (221 / 220) is never taken either way: that pair of runs only shows the
    switch is accepted.  The persistent kernel inside a forward is test_persistent_gemm_whole_model_is_bit_identical below.  attn_out_ln (1341 / 1340) replaces two launches and
    differs from them by the out-projection's summation order in front of one f16 store, the folded LayerNorm of the wide
    depth-wise stack (on / off) by where a stored tensor is rounded: both stay within the bound every mixed16 mel is held to
    against the oracle (2 x the CPU model's fp16 error, test 2 (b)) - of each other."""
    cfg, sd, _, ref, batch, forced = _case(case)
    yh_max, _, _ = _yardstick(case, torch.float16)
    m = _model(cfg, sd, "mixed16")
    base = _cpu(m.forward(batch, **forced))["mel"]
    for off, on in ((1400, 1401), (1402, 1401), (220, 221)):
        m.engine.set_tuning(off)
        try:
            assert torch.equal(_cpu(m.forward(batch, **forced))["mel"], base), (case, off)
        finally:
            m.engine.set_tuning(on)
    m.engine.set_tuning(1340)
    try:
        two = _cpu(m.forward(batch, **forced))["mel"]
    finally:
        m.engine.set_tuning(1341)
    d_attn = float((two - base).abs().max())
    m.engine.set_folded_layernorm(False)
    unfolded = _cpu(m.forward(batch, **forced))["mel"]
    m.engine.set_folded_layernorm(True)
    d_fold = float((unfolded - base).abs().max())
    m.engine.set_deferred_layernorm(False)
    undeferred = _cpu(m.forward(batch, **forced))["mel"]
    m.engine.set_deferred_layernorm(True)
    d_defer = float((undeferred - base).abs().max())
    _report(test="mixed16_dispatch", case=case, attn_out_ln_vs_two_launches=d_attn, folded_vs_passes=d_fold, deferred_vs_launches=d_defer,
            bound=2 * yh_max)
    assert d_attn <= 2 * yh_max and d_fold <= 2 * yh_max and d_defer <= 2 * yh_max, (d_attn, d_fold, d_defer, yh_max)
    e = (undeferred - ref["mel"]).abs()
    assert float(e.max()) <= 2 * yh_max   # the unfused launches meet the same bar against the oracle
    assert torch.equal(_cpu(m.forward(batch, **forced))["mel"], base)


def test_persistent_gemm_whole_model_is_bit_identical():
    """The LightSpeech block (H = 768, depth-wise, deferred + folded LayerNorm) at a size whose decoder GEMMs take the persistent
    kernel in f16 (12 x 1536 frames: 96 row tiles x 3 .. 12 column tiles > 256 CUs; the deferred-statistics epilogue, the residual
    normalised on load, the row-scaled in-projection, ReLU) against the same model with every GEMM one tile per workgroup (knob
    220): the same bits in every output, twice.  The counterpart of tests/test_gpu_configs.py's bf16 test."""
    cfg = Fs2Config(**{**preset("c3").to_dict(), "encoder_layers": 1, "decoder_layers": 2, "variance_nlayers": [2, 2, 2]})
    sd = synth_state_dict(cfg, 2, randomize_norm=True, duration_bias=float(np.log(7.0)), duration_weight_scale=0.0)
    inp = synth_inputs(cfg, 12, 256, seed=99)
    batch = {"phones": torch.from_numpy(inp["phones"]), "speaker": torch.from_numpy(inp["speaker"])}
    m = _model(cfg, sd, "mixed16")
    outs = {}
    try:
        for k in (220, 221, 221):
            m.engine.set_tuning(k)
            outs.setdefault(k, []).append(_cpu(m(batch, inference=True)))
    finally:
        m.engine.set_tuning(221)
    a, b, c = outs[220][0], outs[221][0], outs[221][1]
    assert tuple(b["mel"].shape) == (12, 1536, 80) and bool(torch.isfinite(b["mel"]).all())
    _same(a, b, "one tile per workgroup vs persistent")
    _same(b, c, "persistent, again")
