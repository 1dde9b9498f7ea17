"""The stochastic duration predictor on the device (fs2_sdp_*, fs2_op_rq_spline_inverse, fs2_op_durations_stochastic) against the
reference's fixtures (tests/golden/sdp, tools/gen_golden_sdp.py) and the CPU restatement tests/_sdp_ref.py.

The error bar: e_ref = max |logw - logw64| of a fixture is the reference's own float32 error against its float64 run on the same
noise; the device is held to max |device - logw64| <= 4 e_ref (another summation order, the MFMA's accumulation).  Where there is
no fixture (tile edges, other widths) e_ref is the same figure of tests/_sdp_ref.py in float32 against itself in float64, per case,
and not below 2^-21: one float32 step at the spline's range (its values lie in [-5, 5], steps of 2^-21 from 4 on), under which the
maximum over a handful of rows of ANY float32 evaluation cannot be expected to stay (a lone row can land on the float64 value by
luck).  Durations must be equal exactly: the generator refuses a fixture with exp(logw64) within 5e-5 relative of an integer.

Ratios seen on an MI355X: profiles/sdp.md."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import _sdp_ref as R
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.sdp import StochasticDurationPredictor, durations_stochastic, rq_spline_inverse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdp")
FACTOR = 4.0
E_FLOOR = 2.0 ** -21  # see the docstring


@functools.lru_cache(maxsize=None)
def module_fixture(n):
    z = np.load(os.path.join(GOLDEN, f"module_n{n}.npz"))
    cfg = Fs2Config.from_json(str(z["config_json"]))
    rc = json.loads(str(z["recipe_json"]))
    w = R.sdp_state_dict(cfg, rc["weights_seed"])
    x, pad = R.module_inputs(rc["inputs_seed"])
    assert R.digest(w, x, pad) == str(z["sha256"]), "the synthetic recipe drifted from the fixture"
    return cfg, w, x, pad, {k: z[k] for k in ("noise", "logw", "logw64", "durations")}


@functools.lru_cache(maxsize=None)
def predictor(n, hidden=256):
    cfg = R.module_config(n, hidden)
    seed = {1: 100, 2: 200, 3: 300}[n] if hidden == 256 else 77  # hidden 256: the module fixtures' weights
    w = R.sdp_state_dict(cfg, seed)
    return StochasticDurationPredictor(hidden, 256, 3, n, w, device=DEV), w


def run(p, x, pad, noise):
    out = p(torch.as_tensor(x).to(DEV), torch.as_tensor(pad).to(DEV), torch.as_tensor(noise).to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_module_fixture(n):
    cfg, w, x, pad, fx = module_fixture(n)
    p, _ = predictor(n)
    assert p.launches == (1 if n == 1 else n)  # the conditioning + one per ConvFlow that runs; n = 1: the affine alone
    logw = run(p, x, pad, fx["noise"])
    e_ref = float(np.abs(fx["logw"] - fx["logw64"]).max())
    err = float(np.abs(logw - fx["logw64"]).max())
    print(f"sdp module n={n}: device error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
    assert np.isfinite(logw).all() and (logw[pad] == 0).all()
    assert err <= FACTOR * e_ref
    d = durations_stochastic(torch.as_tensor(logw).to(DEV), torch.as_tensor(pad).to(DEV))
    # the fixture's durations are the bare ceil(exp(.)) rule; no utterance of it trips the zero-duration guard
    assert int(d["guard"].sum()) == 0
    assert np.array_equal(d["dur"].cpu().numpy(), fx["durations"])


def test_spline_fixture():
    z = np.load(os.path.join(GOLDEN, "spline.npz"))
    out = rq_spline_inverse(torch.as_tensor(z["x1"]).to(DEV), torch.as_tensor(z["h29"]).to(DEV), 256).cpu().numpy()
    e_ref = float(np.abs(z["out32"] - z["out64"]).max())
    err = float(np.abs(out - z["out64"]).max())
    print(f"spline: device error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
    assert np.isfinite(out).all()
    outside = np.abs(z["x1"]) > 5.0
    assert np.array_equal(out[outside], z["x1"][outside])  # the tails are the identity, bit for bit
    assert err <= FACTOR * e_ref


def test_spline_pad_rows_and_guards():
    """h = 0 (a pad row's parameters) is the identity spline on equal bins; NaN-free at the bound and for huge logits"""
    x1 = torch.tensor([-5.0, -2.5, 0.0, 1.0, 5.0, 7.0, -9.0], device=DEV)
    out = rq_spline_inverse(x1, torch.zeros(7, 29, device=DEV), 256).cpu().numpy()
    # equal bins, equal heights: delta = 1; derivatives 1e-3 + softplus(0) inside, 1 at the ends: not the identity inside, but
    # monotone, finite, fixed at the knots -5, 0, 5 and the identity outside
    assert np.isfinite(out).all() and (np.diff(out[:6]) > 0).all()
    assert out[0] == -5.0 and abs(out[2]) < 1e-6 and abs(out[4] - 5.0) < 1e-5 and out[5] == 7.0 and out[6] == -9.0
    big = torch.zeros(3, 29, device=DEV)
    big[:, :20] = torch.tensor(np.random.RandomState(0).standard_normal((3, 20)).astype(np.float32) * 3000.0)
    assert np.isfinite(rq_spline_inverse(torch.tensor([-4.0, 0.3, 4.9], device=DEV), big, 256).cpu().numpy()).all()


def edge_lengths(Rt):
    return [1, 2, 13, 14, 27, Rt - 1, Rt, Rt + 1, Rt + 13, Rt + 14, 2 * Rt + 1]


@functools.lru_cache(maxsize=None)
def edge_references(Rt):
    """per length: x, noise, _sdp_ref in float32 and float64 - computed once, shared, never changed"""
    _, w = predictor(2)
    w32, w64 = R.sdp_weights(w, torch.float32), R.sdp_weights(w, torch.float64)
    ref = {}
    for n in edge_lengths(Rt):
        rs = np.random.RandomState(1000 + n)
        x = rs.standard_normal((1, n, 256)).astype(np.float32)
        noise = rs.standard_normal((1, 2, n)).astype(np.float32)
        pad = np.zeros((1, n), bool)
        ref[n] = (x, noise, pad, R.sdp_logw(w32, x, pad, noise).numpy(), R.sdp_logw(w64, x, pad, noise).numpy())
    return ref


def test_tile_edges():
    p, _ = predictor(2)
    Rt = p.tile_rows
    assert Rt >= 28  # a tile finishes more rows than two halos
    ref = edge_references(Rt)
    for n, (x, noise, pad, l32, l64) in ref.items():
        logw = run(p, x, pad, noise)
        e_ref = max(float(np.abs(l32 - l64).max()), E_FLOOR)
        err = float(np.abs(logw - l64).max())
        print(f"sdp tile edge L={n}: device error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
        assert np.isfinite(logw).all() and err <= FACTOR * e_ref, n


def test_batch_invariance_bitwise():
    p, _ = predictor(3)
    Rt = p.tile_rows
    L = 2 * Rt + 1
    lengths = [L, Rt + 1, 14]
    rs = np.random.RandomState(5)
    x = rs.standard_normal((3, L, 256)).astype(np.float32)
    noise = rs.standard_normal((3, 2, L)).astype(np.float32)
    pad = np.arange(L)[None, :] >= np.asarray(lengths)[:, None]
    x[pad] = 7.0  # whatever lies in the pad rows must not matter
    batch = run(p, x, pad, noise)
    assert (batch[pad] == 0).all()
    for b, n in enumerate(lengths):
        alone = run(p, x[b:b + 1, :n], np.zeros((1, n), bool), noise[b:b + 1, :, :n])
        assert np.array_equal(alone[0], batch[b, :n]), (b, n)
        xp = np.concatenate([x[b:b + 1, :n], np.full((1, 7, 256), -3.0, np.float32)], 1)
        zp = np.concatenate([noise[b:b + 1, :, :n], np.ones((1, 2, 7), np.float32)], 2)
        padded = run(p, xp, np.arange(n + 7)[None, :] >= n, zp)
        assert np.array_equal(padded[0, :n], batch[b, :n]) and (padded[0, n:] == 0).all(), (b, n)


def test_one_flow_is_the_affine_alone():
    cfg, w, x, pad, fx = module_fixture(1)
    p, _ = predictor(1)
    logw = run(p, x, pad, fx["noise"])
    t, s = float(w["sdp.flows.0.translation"][0, 0]), float(w["sdp.flows.0.log_scale"][0, 0])
    want = (fx["noise"][:, 1].astype(np.float64) - t) * np.exp(-s)  # channel 0 of the flipped noise
    want[pad] = 0
    e_ref = float(np.abs(fx["logw"] - fx["logw64"]).max())
    assert np.abs(logw - want).max() <= FACTOR * e_ref


def test_other_widths_and_dtypes():
    """H = 64 runs `pre` on 4 k-groups inside the conditioning launch; bf16 / fp16 rows are converted as they are read"""
    p, w = predictor(2, 64)
    rs = np.random.RandomState(9)
    L, lengths = 45, [45, 20]
    x = rs.standard_normal((2, L, 64)).astype(np.float32)
    noise = rs.standard_normal((2, 2, L)).astype(np.float32)
    pad = np.arange(L)[None, :] >= np.asarray(lengths)[:, None]
    l32 = R.sdp_logw(R.sdp_weights(w, torch.float32), x, pad, noise).numpy()
    l64 = R.sdp_logw(R.sdp_weights(w, torch.float64), x, pad, noise).numpy()
    logw = run(p, x, pad, noise)
    assert np.abs(logw - l64).max() <= FACTOR * max(float(np.abs(l32 - l64).max()), E_FLOOR)
    for dt in (torch.bfloat16, torch.float16):
        xr = torch.as_tensor(x).to(dt)
        got = p(xr.to(DEV), torch.as_tensor(pad).to(DEV), torch.as_tensor(noise).to(DEV)).cpu().numpy()
        assert np.array_equal(got, run(p, xr.float().numpy(), pad, noise)), dt


def test_forward_argument_errors():
    p, _ = predictor(2)
    lib, ARG, NOMEM = p.lib, _lib.FS2_ERR_ARG, _lib.FS2_ERR_NOMEM
    x = torch.zeros(1, 4, 256, device=DEV)
    pad = torch.zeros(1, 4, dtype=torch.uint8, device=DEV)
    z = torch.zeros(1, 2, 4, device=DEV)
    out = torch.full((1, 4), 5.0, device=DEV)
    ws = torch.empty(p.workspace_bytes(1, 4), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream()
    assert lib.fs2_sdp_forward(p.handle, _lib.FS2_F32, x, pad, z, out, ws, ws.numel() - 1, 1, 4, st) == NOMEM
    assert lib.fs2_sdp_forward(p.handle, _lib.FS2_F32, None, pad, z, out, ws, ws.numel(), 1, 4, st) == ARG
    assert lib.fs2_sdp_forward(p.handle, 99, x, pad, z, out, ws, ws.numel(), 1, 4, st) == ARG
    assert lib.fs2_sdp_forward(p.handle, _lib.FS2_F32, x, pad, z, out, ws, ws.numel(), 0, 4, st) == ARG
    torch.cuda.synchronize()
    assert (out == 5.0).all()  # nothing was launched


# ---- fs2_op_durations_stochastic
def test_durations_rule_on_a_grid():
    k = np.arange(0, 60)
    vals = np.concatenate([np.log(k[:, None] + np.array([0.25, 0.5, 0.75])[None, :]).ravel(), [-3.0, -0.5, 5.5]]).astype(np.float32)
    logw = torch.as_tensor(vals[None, :]).to(DEV)
    mask = torch.zeros(1, len(vals), dtype=torch.bool, device=DEV)
    d = durations_stochastic(logw, mask)
    want, _ = R.durations_stochastic(vals[None, :])
    assert np.array_equal(d["dur"].cpu().numpy(), want.numpy())
    assert np.array_equal(d["dur"].cpu().numpy()[0, :180], np.repeat(k + 1, 3))
    assert np.array_equal(d["cum"].cpu().numpy()[0], np.cumsum(want.numpy()[0]))
    assert int(d["totals"][0]) == int(want.sum()) and int(d["guard"][0]) == 0


def test_durations_zero_guard_forced_and_limits():
    logw = torch.tensor([[0.0, 1.0, 0.0, 2.0, 0.0, 0.0],      # logw == 0 gives 0; 3 + 8 > 6 // 2: no guard
                         [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],      # all zero: the guard sets the valid entries to 1
                         [-0.1, 0.0, 0.0, 0.0, 0.0, 0.0],     # sum 1 <= 4 // 2 over the four valid entries: the guard
                         [float("nan"), 90.0, -200.0, 0.0, 0.0, 0.0]], device=DEV)  # NaN -> 0, beyond int32 saturates, expf(-200) = 0
    mask = torch.tensor([[0, 0, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1]], dtype=torch.bool, device=DEV)
    d = durations_stochastic(logw, mask)
    dur = d["dur"].cpu().numpy()
    assert dur[0].tolist() == [0, 3, 0, 8, 0, 0] and dur[1].tolist() == [1, 1, 1, 0, 0, 0] and dur[2].tolist() == [1, 1, 1, 1, 0, 0]
    assert d["guard"].cpu().tolist() == [0, 1, 1, 0]
    assert dur[3].tolist() == [0, 2 ** 31 - 1, 0, 0, 0, 0]
    forced = torch.tensor([[2, 0, 5, -1, 0, 0]] * 4, dtype=torch.int32, device=DEV)
    f = durations_stochastic(logw, mask, forced)
    assert f["dur"].cpu().numpy()[1].tolist() == [2, 0, 5, 0, 0, 0] and f["cum"].cpu().numpy()[1].tolist() == [2, 2, 7, 7, 7, 7]
    assert f["totals"].cpu().tolist() == [7] * 4 and f["guard"].cpu().tolist() == [0] * 4


def test_prefix_sums_equal_the_deterministic_rule_for_equal_durations():
    rs = np.random.RandomState(2)
    B, L = 3, 300  # more than one 256-entry round of the scan
    want = rs.randint(1, 9, (B, L)).astype(np.float32)
    mask = torch.as_tensor(np.arange(L)[None, :] >= np.array([300, 257, 40])[:, None]).to(DEV)
    want[mask.cpu().numpy()] = 0
    sto = torch.as_tensor(np.where(want > 0, np.log(np.maximum(want, 1) - 0.5), 0).astype(np.float32)).to(DEV)  # ceil(exp(.)) = want
    det = torch.as_tensor(np.where(want > 0, np.log(want + 1.0), 0).astype(np.float32)).to(DEV)                 # round(exp(.) - 1) = want
    a = durations_stochastic(sto, mask)
    b = {k: torch.empty_like(v) for k, v in a.items()}
    st = _lib.load().fs2_op_durations(det, mask.to(torch.uint8), None, b["dur"], b["cum"], b["totals"], b["guard"], B, L,
                                      torch.cuda.current_stream())
    assert st == 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["dur"].cpu().numpy(), want.astype(np.int32))
