"""FastDiff on the device where tests/test_gpu_fastdiff.py does not look: the bf16 operators alone, the frame-axis tile seam, the
N = 6 and N = 8 schedules, and uneven chunk walks.  Same judges as there: the CPU restatement tests/_fastdiff_ref.py in float64 is the
truth, its float32 run the fp32 yardstick (MARGIN x), its run with bf16 rounding at the storage points the bf16 yardstick (2 x, max-abs
and rms).

The ``seam`` input needs no fixture file: three utterances of 63, 65 and 64 frames (one row short of a 64-row tile, one row into the
second tile, exactly one tile on the frame axis, where the partial tiles of fd_cond_kernel, the nine kernel-predictor convs, the
coarsest DBlock and the hop-8 LVC block live) in a batch padded to T = 66, the longest utterance in the middle, and the pad of every
input filled with large finite values, the output with 7.5: a read or a write past an utterance shows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _fastdiff_ref as R
from _fastdiff_ref import fixture, schedule, weights
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd import fastdiff as FD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
MARGIN = 4  # the fp32 rule of tests/test_gpu_fastdiff.py: |device - truth| <= MARGIN x max(float32 restatement's error, 2^-23 max|truth|)
PRECISIONS = ("fp32", "bf16")
SEAM_LENGTHS, SEAM_T, SEAM_PAD = (63, 65, 64), 66, 1.0e4


@functools.lru_cache(maxsize=None)
def engine(precision):
    return FD.FastDiff(FD.FastDiffConfig(), weights(), precision=precision, device=DEV)


@functools.lru_cache(maxsize=None)
def ref(kind):
    if kind == "f64":
        return R.FastDiffRef(weights(), torch.float64)
    if kind == "f32":
        return R.FastDiffRef(weights(), torch.float32)
    return R.FastDiffRef(weights(), torch.float64, R.bf16_round)


@functools.lru_cache(maxsize=None)
def kidx(precision):
    return FD.kernel_index(precision)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(DEV, dtype)


def host(t):
    return t.float().cpu().numpy()


def errs(a, truth):
    d = np.asarray(a, np.float64) - truth
    return float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))


def fp32_bound(yard, truth):
    return MARGIN * max(yard, EPS32 * float(np.abs(truth).max()))


def within_2x(what, got, truth, model):
    """the bf16 rule: the engine's max-abs and rms error against float64 at most twice the storage-rounded restatement's"""
    eg, ey = errs(got, truth), errs(model, truth)
    print(f"bf16 {what}: engine max {eg[0]:.3e} rms {eg[1]:.3e}; restatement max {ey[0]:.3e} rms {ey[1]:.3e}; "
          f"ratio {eg[0] / ey[0]:.2f} / {eg[1] / ey[1]:.2f}")
    assert eg[0] <= 2 * ey[0] and eg[1] <= 2 * ey[1], (what, eg, ey)


def within_fp32(what, got, truth, y32):
    g, yard = errs(got, truth)[0], errs(y32, truth)[0]
    bound = fp32_bound(yard, truth)
    print(f"fp32 {what}: device {g:.3e}, float32 restatement {yard:.3e}, ratio {g / yard:.2f}")
    assert g <= bound, (what, g, bound)
    return bound


def judge(precision, what, got, out):
    """``out``: {kind: values} of the restatement on the elements ``got`` holds"""
    if precision == "fp32":
        within_fp32(what, got, out["f64"], out["f32"])
    else:
        within_2x(what, got, out["f64"], out["bf16"])


def kinds(precision):
    return ("f64", "f32") if precision == "fp32" else ("f64", "bf16")


# ---- 1. the bf16 operators alone ----
@pytest.mark.parametrize("hop,lengths,T", [(8, (7, 4, 1), 7), (64, (7, 4, 1), 7), (256, (7, 4, 1), 7), (8, (9, 3), 9)])
def test_op_lvc_bf16(hop, lengths, T):
    """fs2_op_lvc in bf16, every element of every layer, with and without ``add``: the bf16 kernel order (32-wide k-steps, one k-step
    per tap), Vec16 / fd_load4 / fd_store4 of bf16 and, at hop 8, the K concatenation.  Inputs are bf16 values, so they are exact for
    the device, float32 and float64 alike; the device accumulates exact products in fp32, gates in fp32 and rounds ONCE to nearest:

        |got - truth| <= 2^-8 |truth| + MARGIN max(float32 restatement's max error, 2^-23 max|truth|)      at every element

    (2^-8: bf16's unit roundoff).  A truncating store errs by up to 2^-7 |truth| and fails; tests/test_fastdiff_cpu.py shows on the
    CPU that the rounded float32 restatement meets the rule and the truncated one does not.  hop 8 with (9, 3) frames of T = 9:
    two tiles, the second with one live half-wave."""
    inp = R.lvc_op_inputs(hop, lengths, T, seed=hop + T, bf16=True)
    y, x, add, K, bias = inp
    B = len(lengths)
    packed = np.zeros((B, T, 24576), np.float32)
    packed[:, :, kidx("bf16").reshape(-1)] = K.reshape(B, T, -1)
    bf = lambda a: dev(a, torch.bfloat16)
    dy, dk, db, dx, da = bf(y), bf(packed), bf(bias.reshape(B, T, 256)), bf(x), bf(add)
    for layer in range(4):
        want = [(R.lvc_op_ref(inp, b, f, hop, layer, torch.float64), R.lvc_op_ref(inp, b, f, hop, layer, torch.float32))
                for b, f in enumerate(lengths)]
        for w, with_add in enumerate((False, True)):
            got = host(FD.lvc(dy, dk, db, dx, da if with_add else None, lengths, hop, layer, precision="bf16"))
            for b, f in enumerate(lengths):
                assert not got[b, f * hop:].any()  # rows past the utterance are not written
            # one yardstick for the launch (the restatement's worst element of any utterance, as test_op_lvc), |truth| per element
            truth = np.concatenate([t64[w].numpy() for t64, _ in want])
            yard = float(np.abs(np.concatenate([t32[w].double().numpy() for _, t32 in want]) - truth).max())
            worst = R.bf16_elementwise_excess(np.concatenate([got[b, :f * hop] for b, f in enumerate(lengths)]), truth, yard, MARGIN)
            print(f"op_lvc bf16 hop {hop} T {T} layer {layer} add {with_add}: worst (error - bound) {worst:.3e}, float32 restatement {yard:.3e}")
            assert worst <= 0, (hop, T, layer, with_add, worst)


@pytest.mark.parametrize("precision,block", [("bf16", 0), ("bf16", 1), ("bf16", 2), ("fp32", 2)])
def test_op_fd_dblock(precision, block):
    """the three DBlocks in bf16 and the coarsest (8 rows per frame, never run alone before) in fp32 too, on the ragged batch"""
    lengths, T = [7, 4, 1], 7
    per_frame, f = (256, 64, 8)[block], (4, 8, 8)[block]
    rs = np.random.RandomState(40 + block)
    x = R.bf16_round(torch.as_tensor(rs.standard_normal((3, T * per_frame, 32)).astype(np.float32))).numpy()
    got = host(engine(precision).dblock(block, dev(x), lengths))
    out = {k: [] for k in kinds(precision)}
    for b, fr in enumerate(lengths):
        n = fr * per_frame
        for k in out:
            out[k].append(ref(k).dblock(block, torch.as_tensor(x[b, :n].T).to(ref(k).dtype)).double().numpy().T)
        assert not got[b, n // f:].any()
    judge(precision, f"op_fd_dblock {block}", np.concatenate([got[b, :fr * per_frame // f] for b, fr in enumerate(lengths)]),
          {k: np.concatenate(v) for k, v in out.items()})


def predictor_case(precision, block, mel, lengths, step, what):
    """predict_kernels against the restatement's kernels and biases (judged apart: their scales differ), zeros past the frames"""
    K, kb = engine(precision).predict_kernels(block, dev(mel), lengths, step)
    K, kb = host(K), host(kb)
    idx = kidx(precision)
    got, out = {"kernels": [], "bias": []}, {k: {"kernels": [], "bias": []} for k in kinds(precision)}
    for b, f in enumerate(lengths):
        f = int(f)
        for kind in out:
            r = ref(kind)
            cond = torch.as_tensor(mel[b, :f]).to(r.dtype).t() + r.step_offsets(step)[block][:, None]
            k, bi = r.predict(block, cond)
            out[kind]["kernels"].append(k.double().numpy().reshape(-1))
            out[kind]["bias"].append(bi.double().numpy().reshape(-1))
        got["kernels"].append(np.moveaxis(K[b, :f][:, idx], 0, -1).reshape(-1))            # (4, 32, 64, 3, f)
        got["bias"].append(kb[b, :f].reshape(f, 4, 64).transpose(1, 2, 0).reshape(-1))     # (4, 64, f)
        assert not K[b, f:].any() and not kb[b, f:].any()
    for part in ("kernels", "bias"):
        judge(precision, f"{what} {part}", np.concatenate(got[part]), {k: np.concatenate(v[part]) for k, v in out.items()})


@pytest.mark.parametrize("block", [0, 1, 2])
def test_kernel_predictor_bf16(block):
    """the chain of cond + 9 convs in bf16 (KE = 32: NKC = 3 for the 96-channel input conv, 2 for the 64-channel ones, the wide
    kernel_conv kernel), mapped back through kernel_index("bf16")"""
    fx = fixture("ragged")
    predictor_case("bf16", block, fx["mel"], fx["lengths"], float(fx["eps_steps"][0]), f"kernel predictor {block} ragged")


# ---- 2. the frame-axis seam ----
@functools.lru_cache(maxsize=None)
def seam():
    """mel (3, 66, 80), noise (3, 3, 66 * 256) (x = noise[0]; all three for inference(N = 3)), pads = SEAM_PAD / -SEAM_PAD"""
    rs = np.random.RandomState(6365)
    B, S = len(SEAM_LENGTHS), SEAM_T * 256
    mel = np.full((B, SEAM_T, 80), SEAM_PAD, np.float32)
    noise = np.full((3, B, S), -SEAM_PAD, np.float32)
    for b, f in enumerate(SEAM_LENGTHS):
        mel[b, :f] = rs.standard_normal((f, 80))
        noise[:, b, :f * 256] = rs.standard_normal((3, f * 256))
    return {"mel": mel, "noise": noise, "lengths": np.asarray(SEAM_LENGTHS, np.int32), "step": float(fixture("ragged")["eps_steps"][0])}


def seam_mask():
    return np.arange(SEAM_T * 256)[None, :] < (np.asarray(SEAM_LENGTHS) * 256)[:, None]


@functools.lru_cache(maxsize=None)
def seam_ref_eps(kind):
    """(valid samples,) float64: the restatement's eps of the three utterances, one evaluation per kind"""
    s = seam()
    return np.concatenate([ref(kind).eps(torch.as_tensor(s["noise"][0, b, :f * 256]), torch.as_tensor(s["mel"][b, :f]), s["step"]).double().numpy()
                           for b, f in enumerate(SEAM_LENGTHS)])


@functools.lru_cache(maxsize=None)
def seam_run(precision):
    """the seam batch on the device, once per precision: eps and the N = 3 waveform, both into 7.5-filled outputs"""
    s, fd = seam(), engine(precision)
    shape = s["noise"].shape[1:]
    eps = fd.denoise(dev(s["noise"][0]), dev(s["mel"]), s["lengths"], s["step"], out=torch.full(shape, 7.5, device=DEV))
    wav = fd.inference(dev(s["mel"]), s["lengths"], N=3, noise=dev(s["noise"]), out=torch.full(shape, 7.5, device=DEV))
    return eps, wav


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seam_denoise(precision):
    """one eps evaluation at 63 / 65 / 64 frames: fp32 under fp32_bound as test_denoise_fp32, bf16 under the 2x rule; nothing is
    written past an utterance and nothing is read there (the pads hold +-1e4)"""
    eps, wav = (host(t) for t in seam_run(precision))
    keep = seam_mask()
    assert (eps[~keep] == 7.5).all() and (wav[~keep] == 7.5).all()
    assert np.isfinite(wav).all() and all(np.abs(wav[b, :f * 256]).max() == 1.0 for b, f in enumerate(SEAM_LENGTHS))
    judge(precision, "denoise seam", eps[keep], {k: seam_ref_eps(k) for k in kinds(precision)})


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seam_utterance_alone_is_bitwise(precision):
    """each utterance as a batch of its own (B = 1, T = its length: no pad at all) = its rows in the padded batch, bit for bit"""
    s, fd = seam(), engine(precision)
    eps, wav = seam_run(precision)
    for b, f in enumerate(SEAM_LENGTHS):
        n = f * 256
        mel1, noise1 = dev(s["mel"][b:b + 1, :f]), dev(s["noise"][:, b:b + 1, :n])
        assert torch.equal(fd.denoise(noise1[0], mel1, None, s["step"])[0], eps[b, :n]), (precision, b)
        assert torch.equal(fd.inference(mel1, None, N=3, noise=noise1)[0], wav[b, :n]), (precision, b)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seam_utterance_of_zero_frames(precision):
    """a fourth utterance of 0 frames: its row of the output is not written, and the other rows keep their bits"""
    s, fd = seam(), engine(precision)
    eps, wav = seam_run(precision)
    mel = np.concatenate([s["mel"], np.full_like(s["mel"][:1], SEAM_PAD)])
    noise = np.concatenate([s["noise"], np.full_like(s["noise"][:, :1], -SEAM_PAD)], axis=1)
    lengths = np.asarray(SEAM_LENGTHS + (0,), np.int32)
    shape = noise.shape[1:]
    e4 = fd.denoise(dev(noise[0]), dev(mel), lengths, s["step"], out=torch.full(shape, 7.5, device=DEV))
    w4 = fd.inference(dev(mel), lengths, N=3, noise=dev(noise), out=torch.full(shape, 7.5, device=DEV))
    assert bool((e4[3] == 7.5).all()) and bool((w4[3] == 7.5).all())
    assert torch.equal(e4[:3], eps) and torch.equal(w4[:3], wav)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seam_kernel_predictor(precision):
    """the frame-axis launches alone: fd_cond_kernel, the nine convs and the wide kernel_conv kernel at 63 / 65 / 64 rows of T = 66"""
    s = seam()
    predictor_case(precision, 0, s["mel"], s["lengths"], s["step"], "kernel predictor 0 seam")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seam_coarsest_dblock(precision):
    """DBlock 2 (8 rows in, one row out per frame) at 63 / 65 / 64 frames; the pad rows of the input hold 1e4"""
    rs = np.random.RandomState(6366)
    x = np.full((3, SEAM_T * 8, 32), SEAM_PAD, np.float32)
    for b, f in enumerate(SEAM_LENGTHS):
        x[b, :f * 8] = R.bf16_round(torch.as_tensor(rs.standard_normal((f * 8, 32)).astype(np.float32))).numpy()
    got = host(engine(precision).dblock(2, dev(x), list(SEAM_LENGTHS)))
    out = {k: [] for k in kinds(precision)}
    for b, f in enumerate(SEAM_LENGTHS):
        for k in out:
            out[k].append(ref(k).dblock(2, torch.as_tensor(x[b, :f * 8].T).to(ref(k).dtype)).double().numpy().T)
        assert not got[b, f:].any()
    judge(precision, "op_fd_dblock 2 seam", np.concatenate([got[b, :f] for b, f in enumerate(SEAM_LENGTHS)]),
          {k: np.concatenate(v) for k, v in out.items()})


# ---- 3. N = 6 and N = 8 ----
def engine_schedule(N):
    arrs = [(C.c_float * 8)() for _ in range(4)]
    assert _lib.load().fs2_fd_schedule(N, *arrs) == _lib.FS2_OK
    return {k: torch.as_tensor(np.asarray(a[:N], np.float32)) for k, a in zip(("beta", "alpha", "sigma", "steps"), arrs)}


@functools.lru_cache(maxsize=None)
def n68_wav(kind, N, own_schedule=False):
    """(B, S) float64: the restatement's inference(N) on ragged_n68 under the reference's recorded schedule or the engine's own"""
    fx = fixture("ragged_n68")
    sched = engine_schedule(N) if own_schedule else schedule(fx, N)
    out = np.zeros(fx["wav_n8"].shape, np.float64)
    for b, f in enumerate(fx["lengths"]):
        n = int(f) * 256
        out[b, :n] = ref(kind).inference(torch.as_tensor(fx["mel"][b, :f]), [torch.as_tensor(fx["noise"][j, b, :n]) for j in range(N)],
                                         sched).double().numpy()
    return out


def n68_run(precision, N):
    fx = fixture("ragged_n68")
    keep = np.arange(fx["wav_n8"].shape[1])[None, :] < (fx["lengths"].astype(np.int64) * 256)[:, None]
    wav = host(engine(precision).inference(dev(fx["mel"]), fx["lengths"], N=N, noise=dev(fx["noise"][:N]),
                                           out=torch.full(fx["wav_n8"].shape, 7.5, device=DEV)))
    assert (wav[~keep] == 7.5).all()  # samples past an utterance's length are untouched
    for b, f in enumerate(fx["lengths"]):
        assert np.abs(wav[b, :int(f) * 256]).max() == 1.0  # peak-normalised over its own samples
    return fx, np.where(keep, wav, 0.0), keep


def test_launch_counts_of_n6_and_n8():
    assert engine("fp32").launches(6) == 6 * 72 + 1 and engine("bf16").launches(8) == 8 * 72 + 1


def test_inference_n8_fp32():
    """the rule of test_inference_fp32_noise_handed_in at N = 8, the reference's record included"""
    fx, wav, _ = n68_run("fp32", 8)
    truth = n68_wav("f64", 8)
    bound = within_fp32("inference ragged N = 8", wav, truth, n68_wav("f32", 8))
    ref_got = float(np.abs(wav - fx["wav_n8"]).max())
    assert ref_got <= bound + float(fx["wav_n8_err64"]), ref_got


def test_inference_n6_fp32():
    """N = 6, where the engine's schedule departs from the reference's by design (one ulp in alpha[4], six in steps[4]:
    tests/test_fastdiff_cpu.py pins it).  The kernels are judged alone, against the restatement under the ENGINE's schedule.  Against
    the reference's record the engine gets, on top of the N = 4 rule, the float64 restatement's own change between the two schedules
    (computed here, printed): the size of the parity departure, which no kernel can undo."""
    fx, wav, _ = n68_run("fp32", 6)
    truth = n68_wav("f64", 6, True)
    bound = within_fp32("inference ragged N = 6, the engine's schedule", wav, truth, n68_wav("f32", 6, True))
    change = float(np.abs(truth - n68_wav("f64", 6)).max())
    ref_got = float(np.abs(wav - fx["wav_n6"]).max())
    print(f"N = 6: float64 restatement, the reference's schedule -> the engine's: max change of the waveform {change:.3e}; "
          f"device vs the reference's record {ref_got:.3e}; the record's own distance to float64 {float(fx['wav_n6_err64']):.3e}")
    assert change > 0  # the departure is there (a schedule equal to the reference's would make this test's allowance idle)
    assert ref_got <= bound + float(fx["wav_n6_err64"]) + change, (ref_got, bound, change)


def test_inference_n6_bf16():
    _, wav, keep = n68_run("bf16", 6)
    within_2x("inference ragged N = 6", wav[keep], n68_wav("f64", 6, True)[keep], n68_wav("bf16", 6, True)[keep])


# ---- 4. uneven chunk walks ----
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("rows", [(0, 1, 2), (0, 1, 2, 1, 0)])
def test_chunks_of_two_are_bitwise(precision, rows):
    """B = 3 walked 2 + 1 and B = 5 (ragged utterances repeated) walked 2 + 2 + 1: the last chunk is smaller than the layout the
    workspace was cut for, and denoise and inference(N = 4) return the bits of the unchunked run"""
    fx, fd = fixture("ragged"), engine(precision)
    rows = list(rows)
    mel, noise, lengths, step = dev(fx["mel"][rows]), dev(fx["noise"][:, rows]), fx["lengths"][rows], float(fx["eps_steps"][0])
    B = len(rows)
    eps = fd.denoise(noise[0], mel, lengths, step)
    wav = fd.inference(mel, lengths, N=4, noise=noise)
    assert torch.isfinite(eps).all() and torch.isfinite(wav).all()
    whole, two = fd.workspace_bytes(B, 7), fd.workspace_bytes(2, 7)
    try:
        fd.set_chunk(2)
        assert fd.workspace_bytes(B, 7) == two < whole
        assert torch.equal(fd.denoise(noise[0], mel, lengths, step), eps)
        assert torch.equal(fd.inference(mel, lengths, N=4, noise=noise), wav)
    finally:
        fd.set_chunk(0)
    assert fd.workspace_bytes(B, 7) == whole
