"""FastDiff on the device (fs2_fd_*, csrc/fastdiff.hip) against the CPU restatement tests/_fastdiff_ref.py in float64 (the truth), with
the restatement's own float32 error as the yardstick, and against the reference's recorded outputs (tests/golden/fastdiff/).

Inputs: the ragged batch (7, 4 and 1 frames, T = 7: a 1-frame utterance is 8 samples under dilations 9 and 27 at the first LVC block
and one row under dilation 4 at the coarsest DBlock; a pad tail behind every utterance but the longest) and one utterance of 70
frames, which spans at least two tiles of every launch (asserted from tile_rows)."""
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
CASES = ("ragged", "long")
EPS32 = 2.0 ** -23
# fp32 rule: |device - truth| <= MARGIN x max(the float32 restatement's own error against float64 on the same input, 2^-23 max|truth|).
# The device sums in MFMA block order and over taps in its own order and uses its own exp / tanh, so it is another float32
# evaluation of the same function; an indexing or masking error is five orders of magnitude larger.
MARGIN = 4


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
def ref_eps(case, kind, i):
    """(B, S) float64: the restatement's eps of every utterance at eps_steps[i], zeros past its samples"""
    fx = fixture(case)
    out = np.zeros(fx["eps_0"].shape, np.float64)
    for b, f in enumerate(fx["lengths"]):
        n = int(f) * 256
        out[b, :n] = ref(kind).eps(torch.as_tensor(fx["noise"][0, b, :n]), torch.as_tensor(fx["mel"][b, :f]), float(fx["eps_steps"][i])).double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def ref_wav(case, kind, N, seeded=False):
    fx = fixture(case)
    noise = torch.as_tensor(fx["noise"])
    if seeded:
        torch.manual_seed(fx["meta"]["run_seed"])
        noise = FD.draw_noise(fx["lengths"], N)
    out = np.zeros(fx["eps_0"].shape, np.float64)
    for b, f in enumerate(fx["lengths"]):
        n = int(f) * 256
        out[b, :n] = ref(kind).inference(torch.as_tensor(fx["mel"][b, :f]), [noise[j, b, :n] for j in range(N)], schedule(fx, N)).double().numpy()
    return out


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(DEV, dtype)


def errs(a, truth):
    d = np.asarray(a, np.float64) - truth
    return float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))


def fp32_bound(yard, truth):
    return MARGIN * max(yard, EPS32 * float(np.abs(truth).max()))


def valid_mask(fx):
    S = fx["eps_0"].shape[1]
    return np.arange(S)[None, :] < (fx["lengths"].astype(np.int64) * 256)[:, None]


def test_long_case_spans_two_tiles_of_every_launch():
    tile = engine("fp32").tile_rows
    assert tile == 64 and engine("fp32").hop == 256
    # the shortest row axis of a launch is the frame axis (kernel predictor, coarsest DBlock): 70 frames > one tile of 64
    assert int(fixture("long")["lengths"][0]) > tile
    assert engine("fp32").launches() == 71 and engine("fp32").launches(4) == 4 * 72 + 1 and engine("bf16").launches(3) == 3 * 72 + 1  # DESIGN §11's list


# ---- operators alone ----
@pytest.mark.parametrize("hop", [8, 64, 256])
def test_op_lvc(hop):
    """kernels and bias differ per frame and per layer: a wrong frame index, a wrong channel order or a zero where a neighbour sample
    belongs at a frame border gives an O(1) error"""
    lengths, T = [7, 4, 1], 7
    rs = np.random.RandomState(hop)
    B, S = 3, T * hop
    y, x, add = (rs.standard_normal((B, S, 32)) for _ in range(3))
    K = rs.standard_normal((B, T, 4, 32, 64, 3)) * (1 / 96) ** 0.5
    bias = rs.standard_normal((B, T, 4, 64)) * 0.3
    f32 = lambda a: a.astype(np.float32)
    y, x, add, K, bias = f32(y), f32(x), f32(add), f32(K), f32(bias)
    idx = FD.kernel_index("fp32").reshape(-1)
    packed = np.zeros((B, T, 24576), np.float32)
    packed[:, :, idx] = K.reshape(B, T, -1)
    for layer, with_add in ((0, True), (3, False), (2, True)):
        got = FD.lvc(dev(y), dev(packed), dev(bias.reshape(B, T, 256)), dev(x), dev(add) if with_add else None, lengths, hop, layer).cpu().numpy()
        worst = yard = top = 0.0
        for b, f in enumerate(lengths):
            n = f * hop
            res = {}
            for dt in (torch.float64, torch.float32):
                t = lambda a: torch.as_tensor(a).to(dt)
                o = R.FastDiffRef.lvc(t(y[b, :n].T), t(K[b, :f, layer]).permute(1, 2, 3, 0), t(bias[b, :f, layer].T), hop)
                v = t(x[b, :n].T) + torch.sigmoid(o[:32]) * torch.tanh(o[32:])
                res[dt] = (v + t(add[b, :n].T) if with_add else v).double().numpy().T
            worst = max(worst, float(np.abs(got[b, :n] - res[torch.float64]).max()))
            yard = max(yard, float(np.abs(res[torch.float32] - res[torch.float64]).max()))
            top = max(top, float(np.abs(res[torch.float64]).max()))
            assert not got[b, n:].any()  # rows past the utterance are not written
        bound = MARGIN * max(yard, EPS32 * top)
        print(f"op_lvc hop {hop} layer {layer}: device {worst:.3e}, float32 restatement {yard:.3e}, bound {bound:.3e}")
        assert worst <= bound, (hop, layer, worst, bound)


@pytest.mark.parametrize("block", [0, 1])
def test_op_fd_dblock(block):
    """factors 4 and 8 on the ragged batch, against the restatement's DBlock in float64"""
    lengths, T = [7, 4, 1], 7
    per_frame, f = (256, 64)[block], (4, 8)[block]
    rs = np.random.RandomState(20 + block)
    x = rs.standard_normal((3, T * per_frame, 32)).astype(np.float32)
    got = engine("fp32").dblock(block, dev(x), lengths).cpu().numpy()
    worst = yard = top = 0.0
    for b, fr in enumerate(lengths):
        n = fr * per_frame
        want = ref("f64").dblock(block, torch.as_tensor(x[b, :n].T).double()).numpy().T
        y32 = ref("f32").dblock(block, torch.as_tensor(x[b, :n].T)).double().numpy().T
        worst = max(worst, float(np.abs(got[b, :n // f] - want).max()))
        yard, top = max(yard, float(np.abs(y32 - want).max())), max(top, float(np.abs(want).max()))
        assert not got[b, n // f:].any()
    bound = MARGIN * max(yard, EPS32 * top)
    print(f"op_fd_dblock {block}: device {worst:.3e}, float32 restatement {yard:.3e}, bound {bound:.3e}")
    assert worst <= bound, (block, worst, bound)


@pytest.mark.parametrize("block", [0, 2])
def test_kernel_predictor(block):
    """kernels and bias against the restatement's, in the reference's (layer, in, out, k) order"""
    fx = fixture("ragged")
    step = float(fx["eps_steps"][0])
    K, kb = engine("fp32").predict_kernels(block, dev(fx["mel"]), fx["lengths"], step)
    K, kb = K.cpu().numpy(), kb.cpu().numpy()
    idx = FD.kernel_index("fp32")
    worst = yard = top = 0.0
    for b, f in enumerate(fx["lengths"]):
        out = {}
        for kind in ("f64", "f32"):
            r = ref(kind)
            cond = torch.as_tensor(fx["mel"][b, :f]).to(r.dtype).t() + r.step_offsets(step)[block][:, None]
            k, bi = r.predict(block, cond)
            out[kind] = (k.double().numpy(), bi.double().numpy())
        got_k = np.moveaxis(K[b, :f][:, idx], 0, -1)          # (4, 32, 64, 3, f)
        got_b = kb[b, :f].reshape(f, 4, 64).transpose(1, 2, 0)  # (4, 64, f)
        worst = max(worst, float(np.abs(got_k - out["f64"][0]).max()), float(np.abs(got_b - out["f64"][1]).max()))
        yard = max(yard, float(np.abs(out["f32"][0] - out["f64"][0]).max()), float(np.abs(out["f32"][1] - out["f64"][1]).max()))
        top = max(top, float(np.abs(out["f64"][0]).max()), float(np.abs(out["f64"][1]).max()))
        assert not K[b, f:].any() and not kb[b, f:].any()
    bound = MARGIN * max(yard, EPS32 * top)
    print(f"kernel predictor {block}: device {worst:.3e}, float32 restatement {yard:.3e}, bound {bound:.3e}")
    assert worst <= bound, (block, worst, bound)


# ---- the network and the sampler, fp32 ----
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("i", [0, 1])
def test_denoise_fp32(case, i):
    fx = fixture(case)
    eps = engine("fp32").denoise(dev(fx["noise"][0]), dev(fx["mel"]), fx["lengths"], float(fx["eps_steps"][i])).cpu().numpy()
    truth, y32 = ref_eps(case, "f64", i), ref_eps(case, "f32", i)
    got, yard = errs(eps, truth)[0], errs(y32, truth)[0]
    bound = fp32_bound(yard, truth)
    print(f"denoise fp32 {case} step {float(fx['eps_steps'][i]):.2f}: device {got:.3e}, float32 restatement {yard:.3e}, ratio {got / yard:.2f}")
    assert got <= bound, (case, i, got, bound)
    assert not eps[~valid_mask(fx)].any()
    ref_got = float(np.abs(eps - fx[f"eps_{i}"]).max())
    assert ref_got <= bound + float(fx[f"eps_{i}_err64"]), (case, i, ref_got)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N", [4, 3])
def test_inference_fp32_noise_handed_in(case, N):
    fx = fixture(case)
    sentinel = torch.full(fx["eps_0"].shape, 7.5, device=DEV)
    wav = engine("fp32").inference(dev(fx["mel"]), fx["lengths"], N=N, noise=dev(fx["noise"][:N]), out=sentinel).cpu().numpy()
    keep = valid_mask(fx)
    assert (wav[~keep] == 7.5).all()  # samples past an utterance's length are untouched
    wav = np.where(keep, wav, 0.0)
    truth, y32 = ref_wav(case, "f64", N), ref_wav(case, "f32", N)
    got, yard = errs(wav, truth)[0], errs(y32, truth)[0]
    bound = fp32_bound(yard, truth)
    print(f"inference fp32 {case} N = {N}: device {got:.3e}, float32 restatement {yard:.3e}, ratio {got / yard:.2f}")
    assert got <= bound, (case, N, got, bound)
    ref_got = float(np.abs(wav - fx[f"wav_n{N}"]).max())
    assert ref_got <= bound + float(fx[f"wav_n{N}_err64"]), (case, N, ref_got)
    for b, f in enumerate(fx["lengths"]):
        assert np.abs(wav[b, :int(f) * 256]).max() == 1.0  # peak-normalised over its own samples


def test_inference_seeded_matches_the_references_run():
    fx = fixture("ragged")
    torch.manual_seed(fx["meta"]["run_seed"])
    wav = engine("fp32").inference(dev(fx["mel"]), fx["lengths"]).cpu().numpy()
    truth, y32 = ref_wav("ragged", "f64", 4, True), ref_wav("ragged", "f32", 4, True)
    bound = fp32_bound(errs(y32, truth)[0], truth)
    assert errs(wav, truth)[0] <= bound
    assert float(np.abs(wav - fx["wav_seeded"]).max()) <= bound + float(fx["wav_n4_err64"])


# ---- batch invariance, bitwise ----
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_invariance_is_bitwise(precision):
    fx, fd = fixture("ragged"), engine(precision)
    mel, noise, step = dev(fx["mel"]), dev(fx["noise"]), float(fx["eps_steps"][0])
    eps = fd.denoise(noise[0], mel, fx["lengths"], step)
    wav = fd.inference(mel, fx["lengths"], N=4, noise=noise)
    assert torch.isfinite(eps).all() and torch.isfinite(wav).all()
    for b, f in enumerate(fx["lengths"]):
        f, n = int(f), int(f) * 256
        e1 = fd.denoise(noise[0, b:b + 1, :n].contiguous(), mel[b:b + 1, :f].contiguous(), None, step)
        w1 = fd.inference(mel[b:b + 1, :f].contiguous(), None, N=4, noise=noise[:, b:b + 1, :n].contiguous())
        assert torch.equal(e1[0], eps[b, :n]) and torch.equal(w1[0], wav[b, :n]), (precision, b)
    try:
        fd.set_chunk(1)  # the batch walked one utterance at a time
        small = fd.workspace_bytes(3, 7)
        assert torch.equal(fd.denoise(noise[0], mel, fx["lengths"], step), eps)
        assert torch.equal(fd.inference(mel, fx["lengths"], N=4, noise=noise), wav)
    finally:
        fd.set_chunk(0)
    assert small < fd.workspace_bytes(3, 7)


# ---- bf16 ----
@pytest.mark.parametrize("case", CASES)
def test_bf16_is_within_2x_of_the_restatement_with_storage_rounding(case):
    """the rule of tests/test_gpu_hifigan_fp16.py: the engine's bf16 error against float64 is at most twice that of the restatement run
    with bf16 rounding at the documented storage points (max-abs and rms)"""
    fx, fd = fixture(case), engine("bf16")
    keep = valid_mask(fx)
    eps = fd.denoise(dev(fx["noise"][0]), dev(fx["mel"]), fx["lengths"], float(fx["eps_steps"][0])).cpu().numpy()
    wav = fd.inference(dev(fx["mel"]), fx["lengths"], N=4, noise=dev(fx["noise"])).cpu().numpy()
    for what, got, truth, model in (("denoise", eps, ref_eps(case, "f64", 0), ref_eps(case, "bf16", 0)),
                                    ("inference", wav, ref_wav(case, "f64", 4), ref_wav(case, "bf16", 4))):
        eg, ey = errs(got[keep], truth[keep]), errs(model[keep], truth[keep])
        print(f"bf16 {what} {case}: engine max {eg[0]:.3e} rms {eg[1]:.3e}; restatement max {ey[0]:.3e} rms {ey[1]:.3e}; "
              f"ratio {eg[0] / ey[0]:.2f} / {eg[1] / ey[1]:.2f}")
        assert eg[0] <= 2 * ey[0] and eg[1] <= 2 * ey[1], (case, what, eg, ey)


# ---- boundary ----
def test_speech_generator_takes_fastdiff():
    from lightningfastspeech2_amd.config import Fs2Config
    from lightningfastspeech2_amd.model import FastSpeech2
    from lightningfastspeech2_amd.synthesis import SpeechGenerator
    from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict as fs2_sd
    cfg = Fs2Config(n_phones=40, encoder_hidden=64, decoder_hidden=64, encoder_head=2, decoder_head=2,
                    encoder_layers=2, decoder_layers=2, encoder_kernel_sizes=[3, 5], decoder_kernel_sizes=[5, 3],
                    encoder_conv_filter_size=128, decoder_conv_filter_size=128, encoder_depthwise_conv=False,
                    decoder_depthwise_conv=False, variance_filter_size=64, variance_depthwise_conv=False,
                    variance_nlayers=[2, 2, 2], duration_filter_size=64, duration_depthwise_conv=False, n_mels=80)
    model = FastSpeech2(cfg, fs2_sd(cfg, 3, randomize_norm=True, duration_bias=1.3), precision="fp32", device=DEV)
    inp = synth_inputs(cfg, 3, 5, seed=7, lengths=[5, 2, 3])
    batch = {"phones": torch.from_numpy(inp["phones"]), "speaker": torch.from_numpy(inp["speaker"])}
    fd = engine("fp32")
    gen = SpeechGenerator(model, fd)
    torch.manual_seed(99)
    out = gen.generate_samples(batch)
    res = model(batch, inference=True)
    frames = (~res["tgt_mask"]).sum(1).cpu().tolist()
    torch.manual_seed(99)
    want = fd.inference(res["mel"], torch.as_tensor(frames)).cpu().numpy()
    assert len(out["audios"]) == 3
    for b, a in enumerate(out["audios"]):
        assert a.dtype == np.float32 and a.shape == (frames[b] * 256,)
        assert np.array_equal(a, want[b, :frames[b] * 256]) and np.abs(a).max() == 1.0  # the samples themselves, unquantised
    pipe = gen.pipeline(2)
    torch.manual_seed(99)
    got = pipe.submit(batch) + pipe.drain()
    pipe.close()
    assert len(got) == 1 and all(np.array_equal(a, b) for a, b in zip(got[0]["audios"], out["audios"]))
    with pytest.raises(ValueError):
        gen.generate_samples(batch, audio_dtype="int16")


def test_errors_are_judged_on_the_host():
    fx, fd = fixture("ragged"), engine("fp32")
    lib, h = fd.lib, fd.handle
    mel, noise = dev(fx["mel"]), dev(fx["noise"])
    with pytest.raises(RuntimeError, match="tabulated schedules"):
        fd.inference(mel, fx["lengths"], N=5, noise=torch.zeros(5, 3, 7 * 256))
    ws = torch.empty(fd.workspace_bytes(3, 7), dtype=torch.uint8, device=DEV)
    wav = torch.zeros(3, 7 * 256, device=DEV)
    stream = torch.cuda.current_stream()
    assert lib.fs2_fd_sample(h, mel, None, noise, 4, wav, ws, ws.numel() - 256, 3, 7, stream) == _lib.FS2_ERR_NOMEM
    assert b"needed" in lib.fs2_fd_last_error(h)
    assert lib.fs2_fd_denoise(h, noise, mel, None, C.c_float(3.0), wav, None, 0, 3, 7, stream) == _lib.FS2_ERR_NOMEM
    assert lib.fs2_fd_sample(h, mel, None, noise, 200, wav, ws, ws.numel(), 3, 7, stream) == _lib.FS2_ERR_SHAPE
    assert lib.fs2_fd_sample(h, None, None, noise, 4, wav, ws, ws.numel(), 3, 7, stream) == _lib.FS2_ERR_ARG
    torch.cuda.synchronize()
    assert not wav.any()  # nothing was launched
    with pytest.raises(ValueError):
        FD.FastDiff(FD.FastDiffConfig(), weights(), precision="fp16", device=DEV)
    bad = dict(weights())
    bad["final_conv.0.weight"] = np.zeros((1, 32, 5), np.float32)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        FD.FastDiff(FD.FastDiffConfig(), bad, precision="fp32", device=DEV)
