"""Augmentation on the device (csrc/augment.hip) against the restated definitions of tests/_augment_ref.py.

Exact cases are compared bit for bit.  Numeric cases follow the rule of test_gpu_analysis.py: max |device - float64| over an utterance
is at most 2x the sequential float32 chain's own error against float64 on that utterance (the chain's figure asserted > 0 where the
utterance has sums to round, so the comparison cannot pass vacuously).  Packed buffers start 3 samples in (odd offsets on purpose),
are followed by NaN in `in` (never read) and by NaN sentinels in `out` (never written)."""
import numpy as np
import pytest
import torch

import _augment_ref as ref
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.augment import (DeviceAugment, GaussianSNR, Resample, RoomImpulse, resample_params, resample_table,
                                              resampled_length, synthetic_rir, wav_add_noise, wav_convolve, wav_resample)
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.hifigan import HifiGan, HifiGanConfig, synth_state_dict
from lightningfastspeech2_amd.model import FastSpeech2
from lightningfastspeech2_amd.synthesis import SpeechGenerator
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict as fs2_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
RATIOS = [(22050, 16000), (1, 2), (2, 1), (22050, 24000), (48000, 22050)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tile():
    return int(_lib.load().fs2_op_wav_convolve_tile())


def utterances(lengths, seed):
    rng = np.random.default_rng(seed)
    return [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lengths]


def seam_lengths():
    t = tile()
    return [0, 1, t - 1, t, 2 * t + 17]


def split(out, off):
    out, off = out.cpu().numpy(), off.cpu().numpy()
    assert off[0] == 0 and (np.diff(off) >= 0).all()
    assert np.isnan(out[off[-1]:]).all(), "out beyond out_offsets[B] was written"
    return [out[off[b]:off[b + 1]] for b in range(len(off) - 1)], off


def bank_of(rirs):
    R_max = max(len(h) for h in rirs)
    bank = np.zeros((len(rirs), R_max), np.float32)
    for i, h in enumerate(rirs):
        bank[i, :len(h)] = h
    return dev(bank), dev(np.array([len(h) for h in rirs], np.int32)), R_max


def convolve(utts, rirs, index, mode, lead=3):
    buf, off = ref.pack(utts, lead=lead, tail=GUARD)
    bank, lens, R_max = bank_of(rirs)
    B, max_len = len(utts), max(len(u) for u in utts)
    worst = max_len if mode == "same" else max_len + R_max - 1
    out = torch.full((B * worst + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    got, out_off, m = wav_convolve(dev(buf), dev(off), max_len, bank, lens, dev(np.asarray(index, np.int32)), mode, out=out)
    torch.cuda.synchronize()
    assert m == worst
    return split(got, out_off)[0]


def resample(utts, rates, lead=3):
    orig, new, width, K = resample_params(*rates)
    buf, off = ref.pack(utts, lead=lead, tail=GUARD)
    B, max_len = len(utts), max(len(u) for u in utts)
    worst = resampled_length(max_len, orig, new)
    out = torch.full((B * worst + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    tab = dev(resample_table(*rates).astype(np.float32))
    got, out_off, m = wav_resample(dev(buf), dev(off), max_len, tab, orig, new, width, out=out)
    torch.cuda.synchronize()
    assert m == worst
    return split(got, out_off)[0]


def add_noise(utts, zs, snr, lead=3, in_place=False):
    buf, off = ref.pack(utts, lead=lead, tail=GUARD)
    zbuf, _ = ref.pack(zs, lead=lead, tail=GUARD)
    x = dev(buf)
    out = x if in_place else torch.full_like(x, float("nan"))
    got, scales = wav_add_noise(x, dev(off), max((len(u) for u in utts), default=0), dev(zbuf), dev(np.asarray(snr, np.float32)), out=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if not in_place:
        assert np.isnan(got[:lead]).all() and np.isnan(got[off[-1]:]).all(), "out outside the utterances was written"
    return [got[off[b]:off[b + 1]] for b in range(len(utts))], scales.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def within_chain(got, want64, chain32, what, need_positive):
    if len(want64) == 0:
        assert len(got) == 0, what
        return
    d, m = np.abs(got.astype(np.float64) - want64).max(), np.abs(chain32.astype(np.float64) - want64).max()
    print(f"{what}: device {d:.3e} chain {m:.3e} (peak {np.abs(want64).max():.3e})")
    assert np.isfinite(got).all(), what
    if need_positive:
        assert m > 0, what
    assert d <= 2 * m, (what, d, m)


# ---- convolution
def test_convolve_exact_cases():
    utts = utterances(seam_lengths(), 1)
    delta5 = np.zeros(6, np.float32)
    delta5[5] = 1.0
    h31 = synthetic_rir(31, 0.2, 2)
    rirs = [np.ones(1, np.float32), delta5, h31]
    B = len(utts)
    for mode in ("same", "full"):
        unit = convolve(utts, rirs, [0] * B, mode)
        none = convolve(utts, rirs, [-1] * B, mode)
        shift = convolve(utts, rirs, [1] * B, mode)
        for u, a, c, s in zip(utts, unit, none, shift):
            assert same_bits(a, u) and same_bits(c, u)  # h = [1] (R = 1: FULL keeps n samples too) and "no response"
            want = np.concatenate([np.zeros(5, np.float32), u])[:len(u) if mode == "same" else len(u) + 5] if len(u) else u
            assert same_bits(s, want)
    full, same = convolve(utts, rirs, [2] * B, "full"), convolve(utts, rirs, [2] * B, "same")
    for u, f, s in zip(utts, full, same):
        assert len(s) == len(u) and len(f) == (len(u) + 30 if len(u) else 0) and same_bits(f[:len(u)], s)
    # mixed indices in one batch, an index past the bank counts as "none"
    mixed = convolve(utts, rirs, [2, 0, -1, 1, 7], "full")
    assert same_bits(mixed[2], utts[2]) and same_bits(mixed[4], utts[4]) and same_bits(mixed[3][5:], utts[3])


@pytest.mark.parametrize("R", [2, 31, 33, 700])
def test_convolve_numeric(R):
    utts = utterances(seam_lengths() + [100], 3)
    h = synthetic_rir(R, 4.0 / R, 10 + R)
    rirs = [synthetic_rir(700, 0.01, 5), h]  # R_max = 700 whatever R is
    got = convolve(utts, rirs, [1] * len(utts), "full")
    for u, g in zip(utts, got):
        assert len(g) == (len(u) + R - 1 if len(u) else 0)
        within_chain(g, ref.convolve_f64(u, h, "full"), ref.convolve_chain32(u, h, "full"), f"R={R} n={len(u)}", len(u) >= 32)


def test_convolve_longest_response():
    (u,) = utterances([20000], 4)
    h = synthetic_rir(16384, 5.0 / 16384, 6)
    (g,) = convolve([u], [h], [0], "full")
    assert len(g) == 20000 + 16383
    within_chain(g, ref.convolve_f64(u, h, "full"), ref.convolve_chain32(u, h, "full"), "R=16384 n=20000", True)


# ---- resampler
@pytest.mark.parametrize("rates", RATIOS)
def test_resample(rates):
    orig, new, width, K = resample_params(*rates)
    seam = int(_lib.load().fs2_op_wav_resample_tile(orig, new, width))
    assert seam > 0 and seam % (32 * orig) == 0
    lengths = [0, 1, orig - 1, orig + 1, 5 * orig + 3, seam - 1, seam + 1]
    utts = utterances(lengths, 7)
    got = resample(utts, rates)
    for u, g in zip(utts, got):
        assert len(g) == -(-new * len(u) // orig)  # exact lengths
        within_chain(g, ref.resample_f64(u, *rates), ref.resample_chain32(u, *rates), f"{rates} n={len(u)}", len(u) >= 32)


# ---- noise
def test_noise():
    utts = utterances(seam_lengths(), 8)
    zs = utterances(seam_lengths(), 9)
    snr = [10.0, 3.0, np.inf, 0.5, 30.0]
    got, scales = add_noise(utts, zs, snr)
    for u, z, s, g, sc in zip(utts, zs, snr, got, scales):
        want = ref.noise_scale_f64(u, s)
        assert abs(float(sc) - want) <= np.spacing(np.float32(want)), (len(u), s, sc, want)  # within one float32 ulp
        assert same_bits(g, u if np.isinf(s) else ref.add_noise_f32(u, z, sc))
    assert scales[0] == 0.0 and scales[2] == 0.0 and (scales[[1, 3, 4]] > 0).all()
    again, scales2 = add_noise(utts, zs, snr, in_place=True)
    assert np.array_equal(scales, scales2) and all(same_bits(a, b) for a, b in zip(again, got))
    # 16-byte aligned utterances take the wide path: the same samples either way
    wide, scales3 = add_noise(utts, zs, snr, lead=0)
    assert np.array_equal(scales, scales3) and all(same_bits(a, b) for a, b in zip(wide, got))


# ---- batch invariance: every utterance alone at offset 0 equals its slice of the batched run, bit for bit
def test_batch_invariance():
    t = tile()
    utts = utterances([t + 5, 1, 2 * t + 17, 300, t - 1], 12)
    rirs = [synthetic_rir(33, 0.1, 1), synthetic_rir(700, 0.01, 2)]
    index = [1, 0, 0, 1, -1]
    for mode in ("same", "full"):
        batched = convolve(utts, rirs, index, mode)
        for u, i, want in zip(utts, index, batched):
            assert same_bits(convolve([u], rirs, [i], mode, lead=0)[0], want), (mode, len(u))
    rates = (22050, 16000)
    batched = resample(utts, rates)
    for u, want in zip(utts, batched):
        assert same_bits(resample([u], rates, lead=0)[0], want), len(u)
    zs = utterances([len(u) for u in utts], 13)
    snr = [10.0, 20.0, 5.0, np.inf, 0.0]
    batched, scales = add_noise(utts, zs, snr)
    for u, z, s, want, sc in zip(utts, zs, snr, batched, scales):
        alone, sc1 = add_noise([u], [z], [s], lead=0)
        assert same_bits(alone[0], want) and sc1[0] == sc


# ---- end to end: the tiny model and vocoder of test_gpu_speech_pipeline.py
VOC = HifiGanConfig(upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=128,
                    resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 2, 3], [1, 3, 5]])
BATCHES = [(5, 12, [12, 8, 3]), (6, 9, [9, 1, 4, 9]), (7, 5, [5, 2])]


@pytest.fixture(scope="module")
def model():
    cfg = Fs2Config(n_phones=40, encoder_hidden=64, decoder_hidden=64, encoder_head=2, decoder_head=2,
                    encoder_layers=2, decoder_layers=2, encoder_kernel_sizes=[3, 5], decoder_kernel_sizes=[5, 3],
                    encoder_conv_filter_size=128, decoder_conv_filter_size=128, encoder_depthwise_conv=False,
                    decoder_depthwise_conv=False, variance_filter_size=64, variance_depthwise_conv=False,
                    variance_nlayers=[2, 2, 2], duration_filter_size=64, duration_depthwise_conv=False, n_mels=80)
    return FastSpeech2(cfg, fs2_sd(cfg, 3, randomize_norm=True, duration_bias=1.3), precision="fp32", device=DEV)


@pytest.fixture(scope="module")
def vocoder():
    return HifiGan(VOC, synth_state_dict(VOC, 4), precision="fp32")


def batch_of(model, seed, L, lengths):
    inp = synth_inputs(model.cfg, len(lengths), L, seed=seed, lengths=lengths)
    return {"phones": torch.from_numpy(inp["phones"]), "speaker": torch.from_numpy(inp["speaker"])}


def make_aug(seed=11):
    rirs = [synthetic_rir(40, 0.1, 1), synthetic_rir(9, 0.5, 2)]
    return DeviceAugment([Resample(22050, 16000), RoomImpulse(rirs, p=0.5), GaussianSNR(5.0, 30.0, p=0.5)], seed=seed, device=DEV)


def by_hand(model, vocoder, aug, batch):
    result = model(batch, inference=True)
    lengths = (~result["tgt_mask"]).sum(dim=1).to(torch.int32)
    packed, offsets = vocoder.synthesize_packed(result["mel"], lengths, "float32")
    packed, offsets, fs = aug(packed, offsets, 22050, result["mel"].shape[1] * vocoder.hop)
    torch.cuda.synchronize()
    off, flat = offsets.cpu().numpy(), packed.cpu().numpy()
    return fs, [flat[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def test_generate_samples_with_augmentations(model, vocoder):
    gen = SpeechGenerator(model, vocoder, augmentations=make_aug())
    hand = make_aug()
    plain = SpeechGenerator(model, vocoder)
    changed = 0
    for spec in BATCHES:  # consecutive calls: the generators of both sides advance alike
        out = gen.generate_samples(batch_of(model, *spec))
        fs, want = by_hand(model, vocoder, hand, batch_of(model, *spec))
        assert out["fs"] == fs == 16000 and len(out["audios"]) == len(want)
        assert all(same_bits(a, b) for a, b in zip(out["audios"], want))
        base = plain.generate_samples(batch_of(model, *spec))
        assert base["fs"] == 22050
        for a, b in zip(out["audios"], base["audios"]):
            assert len(a) == -(-320 * len(b) // 441)
        changed += sum(len(a) for a in out["audios"])
    assert changed > 0
    with pytest.raises(ValueError):
        gen.generate_samples(batch_of(model, *BATCHES[0]), audio_dtype="int16")
    with pytest.raises(ValueError):
        gen.pipeline(audio_dtype="int16")


def test_pipeline_with_augmentations_equals_generate_samples(model, vocoder):
    want = []
    seq = SpeechGenerator(model, vocoder, augmentations=make_aug(5))
    for spec in BATCHES:
        want.append(seq.generate_samples(batch_of(model, *spec)))
    pipe = SpeechGenerator(model, vocoder, augmentations=make_aug(5)).pipeline(2)
    got = []
    try:
        for spec in BATCHES:
            for o in pipe.submit(batch_of(model, *spec)):
                got.append((o["fs"], [a.copy() for a in o["audios"]]))
        for o in pipe.drain():
            got.append((o["fs"], [a.copy() for a in o["audios"]]))
    finally:
        pipe.close()
    assert len(got) == len(want)
    for (fs, audios), w in zip(got, want):
        assert fs == w["fs"] == 16000 and len(audios) == len(w["audios"])
        assert all(same_bits(a, b) for a, b in zip(audios, w["audios"]))


def test_no_augmentations_is_todays_output(model, vocoder):
    gen = SpeechGenerator(model, vocoder, augmentations=None)
    batch = batch_of(model, *BATCHES[0])
    result = model(batch, inference=True)
    lengths = (~result["tgt_mask"]).sum(dim=1).to(torch.int32)
    i16 = (vocoder.synthesize(result["mel"], lengths).cpu().numpy() * 32768.0).astype("int16")
    want = [i16[b, :int(n) * vocoder.hop].astype(np.float32) / 32767.0 for b, n in enumerate(lengths.tolist())]
    out = gen.generate_samples(batch)
    assert out["fs"] == 22050 and all(same_bits(a, b) for a, b in zip(out["audios"], want))
    out16 = gen.generate_samples(batch, audio_dtype="int16")
    assert all(a.dtype == np.int16 for a in out16["audios"])
