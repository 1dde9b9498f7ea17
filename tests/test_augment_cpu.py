"""Augmentation without a GPU: the resampler's table and lengths, the restated definitions, the host's random plan, every refusal the
three entry points answer before a device call, and the generator's argument check."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import _augment_ref as ref
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.augment import (DeviceAugment, GaussianSNR, Resample, RoomImpulse, resample_params, resample_table,
                                              resampled_length, synthetic_rir)
from lightningfastspeech2_amd.synthesis import SpeechGenerator

RATIOS = {(22050, 16000): (441, 320, 9, 459), (1, 2): (1, 2, 7, 15), (2, 1): (2, 1, 13, 28), (22050, 24000): (147, 160, 7, 161),
          (48000, 22050): (320, 147, 14, 348)}


@pytest.mark.parametrize("rates", list(RATIOS))
def test_table_shape(rates):
    orig, new, width, K = RATIOS[rates]
    assert resample_params(*rates) == (orig, new, width, K)
    # the definition, term by term, for a few entries
    tab = resample_table(*rates)
    assert tab.shape == (new, K) and tab.dtype == np.float64
    base = min(orig, new) * 0.99
    assert width == math.ceil(6 * orig / base) and K == 2 * width + orig
    for p, q in [(0, 0), (0, width), (new - 1, K - 1), (new // 2, K // 2)]:
        t = min(max((-p / new + (q - width) / orig) * base, -6.0), 6.0)
        want = (1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)) * math.cos(math.pi * t / 12) ** 2 * base / orig
        assert abs(tab[p, q] - want) <= 1e-15
    assert Resample(*rates).K == K


def test_resampled_tone_and_lengths():
    fs, fs2 = 22050, 16000
    orig, new, width, K = resample_params(fs, fs2)
    x = np.sin(2 * np.pi * 1000.0 * np.arange(4 * fs // 10) / fs)
    y = ref.resample_f64(x, fs, fs2, tab32=resample_table(fs, fs2).astype(np.float32))
    want = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / fs2)
    edge = 2 * width
    err = np.abs(y - want)[edge:-edge].max()
    print(f"1 kHz tone 22050 -> 16000: interior max error {err:.3e}")
    assert err <= 1e-3
    for n in (0, 1, orig - 1, orig, orig + 1):
        m = math.ceil(new * n / orig)
        assert resampled_length(n, orig, new) == m
        xs = np.random.default_rng(n).standard_normal(n)
        assert len(ref.resample_f64(xs, fs, fs2)) == m and len(ref.resample_chain32(xs, fs, fs2)) == m
    # the chain is the same sum in float32
    xs = np.random.default_rng(1).standard_normal(3 * orig + 5)
    d = np.abs(ref.resample_chain32(xs, fs, fs2) - ref.resample_f64(xs.astype(np.float32), fs, fs2)).max()
    assert 0 < d < 1e-5


def test_convolution_restatements():
    x = np.random.default_rng(2).standard_normal(300).astype(np.float32)
    h = synthetic_rir(31, 0.1, 3)
    assert h.dtype == np.float32 and h.shape == (31,) and h[0] == 1.0
    assert np.array_equal(synthetic_rir(31, 0.1, 3), h)
    full, same = ref.convolve_f64(x, h, "full"), ref.convolve_f64(x, h, "same")
    assert len(full) == 330 and len(same) == 300 and np.array_equal(full[:300], same)
    t = 100
    assert abs(full[t] - sum(float(h[k]) * float(x[t - k]) for k in range(31))) < 1e-12
    d = np.abs(ref.convolve_chain32(x, h, "full") - full).max()
    assert 0 < d < 1e-5
    assert len(ref.convolve_f64(x[:0], h, "full")) == 0


def test_plan_is_reproducible_and_p_is_honoured():
    rirs = [synthetic_rir(8, 0.5, i) for i in range(3)]
    stages = lambda p: [Resample(22050, 16000), RoomImpulse(rirs, p=p), GaussianSNR(5.0, 30.0, p=p)]
    a, b = DeviceAugment(stages(0.5), seed=7), DeviceAugment(stages(0.5), seed=7)
    for B in (4, 9):  # consecutive calls continue the same generator
        pa, pb = a.plan(B), b.plan(B)
        assert pa[0] is None and pb[0] is None
        for x, y in zip(pa[1:], pb[1:]):
            assert all(np.array_equal(x[k], y[k]) for k in ("apply", "rir", "snr"))
    other = DeviceAugment(stages(0.5), seed=8).plan(64)
    mine = DeviceAugment(stages(0.5), seed=7).plan(64)
    assert not np.array_equal(other[1]["apply"], mine[1]["apply"])
    assert 0 < mine[1]["apply"].sum() < 64 and 0 < mine[2]["apply"].sum() < 64
    # the documented order of draws: per random stage, per utterance: random(), integers(n_rir), uniform(lo, hi)
    rng = np.random.default_rng(7)
    for pl, (n_rir, lo, hi) in zip(mine[1:], [(3, 0.0, 1.0), (1, 5.0, 30.0)]):
        for i in range(64):
            u, r, v = rng.random(), int(rng.integers(n_rir)), rng.uniform(lo, hi)
            assert pl["apply"][i] == (u < 0.5)
            if n_rir == 3:
                assert pl["rir"][i] == (r if u < 0.5 else -1) and np.isposinf(pl["snr"][i])
            else:
                assert pl["rir"][i] == -1 and (pl["snr"][i] == np.float32(v) if u < 0.5 else np.isposinf(pl["snr"][i]))
    never, always = DeviceAugment(stages(0.0), seed=1).plan(32), DeviceAugment(stages(1.0), seed=1).plan(32)
    assert not never[1]["apply"].any() and (never[1]["rir"] == -1).all() and np.isposinf(never[2]["snr"]).all()
    assert always[1]["apply"].all() and ((always[1]["rir"] >= 0) & (always[1]["rir"] < 3)).all()
    assert always[2]["apply"].all() and ((always[2]["snr"] >= 5.0) & (always[2]["snr"] <= 30.0)).all()
    # equal rates drop the stage; the chain's rate and worst-case length
    aug = DeviceAugment([Resample(16000, 16000), Resample(22050, 16000), RoomImpulse(rirs, mode="full")])
    assert len(aug.stages) == 2 and aug.out_fs(22050) == 16000 and aug.out_len(441) == 320 + 7
    with pytest.raises(ValueError):
        aug.out_fs(16000)
    with pytest.raises(ValueError):
        Resample(22050, 22051)  # K far beyond 1024
    with pytest.raises(ValueError):
        RoomImpulse([np.zeros(16385, np.float32)])


P = 64  # a non-null pointer that is never dereferenced: every refusal below is answered on the host


def _resample(lib, **kw):
    a = dict(inp=P, off=P, B=2, max_len=1000, tab=P, orig=441, new=320, width=9, out=P, cap=2 * 726, out_off=P)
    a.update(kw)
    return lib.fs2_op_wav_resample(a["inp"], a["off"], a["B"], a["max_len"], a["tab"], a["orig"], a["new"], a["width"], a["out"],
                                   a["cap"], a["out_off"], None)


def _convolve(lib, **kw):
    a = dict(inp=P, off=P, B=2, max_len=1000, rir=P, rir_len=P, rir_index=P, n_rir=3, R_max=700, mode=_lib.FS2_CONV_SAME, out=P,
             cap=2000, out_off=P)
    a.update(kw)
    return lib.fs2_op_wav_convolve(a["inp"], a["off"], a["B"], a["max_len"], a["rir"], a["rir_len"], a["rir_index"], a["n_rir"],
                                   a["R_max"], a["mode"], a["out"], a["cap"], a["out_off"], None)


def _noise(lib, **kw):
    a = dict(inp=P, off=P, B=2, max_len=1000, z=P, snr=P, ws=P, ws_bytes=1 << 20, out=P, scales=P)
    a.update(kw)
    return lib.fs2_op_wav_add_noise(a["inp"], a["off"], a["B"], a["max_len"], a["z"], a["snr"], a["ws"], a["ws_bytes"], a["out"],
                                    a["scales"], None)


def test_refusals_are_answered_on_the_host():
    lib = _lib.load()
    ARG, SHAPE, NOMEM = _lib.FS2_ERR_ARG, _lib.FS2_ERR_SHAPE, _lib.FS2_ERR_NOMEM
    assert lib.fs2_op_wav_convolve_tile() > 0 and lib.fs2_op_wav_convolve_tile.restype is C.c_int32
    for k in ("inp", "off", "tab", "out", "out_off"):
        assert _resample(lib, **{k: None}) == ARG, k
    assert _resample(lib, B=0) == ARG and _resample(lib, max_len=-1) == ARG and _resample(lib, orig=0) == ARG
    assert _resample(lib, cap=2 * 726 - 1) == ARG                      # ceil(320 * 1000 / 441) = 726 per utterance
    assert _resample(lib, new=641, cap=1 << 40) == SHAPE               # new > 640
    assert _resample(lib, orig=1007, width=9, cap=1 << 40) == SHAPE    # K = 1025
    assert _resample(lib, max_len=(1 << 30) + 1, cap=1 << 60) == SHAPE
    for k in ("inp", "off", "rir", "rir_len", "rir_index", "out", "out_off"):
        assert _convolve(lib, **{k: None}) == ARG, k
    assert _convolve(lib, mode=2) == ARG and _convolve(lib, mode=-1) == ARG
    assert _convolve(lib, n_rir=0) == ARG and _convolve(lib, R_max=0) == ARG and _convolve(lib, B=-3) == ARG
    assert _convolve(lib, R_max=16385) == SHAPE
    assert _convolve(lib, cap=1999) == ARG
    assert _convolve(lib, mode=_lib.FS2_CONV_FULL, cap=2 * (1000 + 699) - 1) == ARG   # FULL: max_len + R_max - 1 per utterance
    for k in ("inp", "off", "z", "snr", "ws", "out", "scales"):
        assert _noise(lib, **{k: None}) == ARG, k
    assert _noise(lib, B=0) == ARG
    need = lib.fs2_op_wav_add_noise_ws_bytes(2, 1000)
    assert need > 0 and need % 8 == 0 and lib.fs2_op_wav_add_noise_ws_bytes(4, 1000) == 2 * need
    assert _noise(lib, ws_bytes=need - 1) == NOMEM


def test_int16_with_augmentations_is_refused():
    model = SimpleNamespace(eval=lambda: None, hparams=SimpleNamespace(sampling_rate=22050))
    aug = DeviceAugment([Resample(22050, 16000)])
    gen = SpeechGenerator(model, SimpleNamespace(device="cuda:0"), augmentations=aug)
    assert gen.fs == 16000 and SpeechGenerator(model, SimpleNamespace()).fs == 22050
    with pytest.raises(ValueError, match="int16"):
        gen.generate_samples({}, audio_dtype="int16")
