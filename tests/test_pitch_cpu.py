"""The F0 tracker without a device: the definition itself (tests/_pitch_ref.py, float64), the condition the GPU file's bars rest on,
the header and what the C entries refuse on the host alone.

The cap.  tests/test_gpu_pitch.py holds the device's decisions to float64's on every frame that is not fragile at E = 2 E_32
(_pitch_ref.fragile); here every case it runs is shown to have at most 2 % fragile frames, with the float64 definition and E_32 alone,
so the choice of signals is verified without a GPU.  Seen here: E_32 = 1.4e-6 ... 1.5e-5, no fragile frame in any of the five cases.

The definition.  On noiseless harmonic tones every interior frame's float64 f0 lies within 1 % of the true fundamental - YIN's
published behaviour, a bound on the definition: seen 1e-5 ... 0.31 %, the largest on the 4 kHz geometry's 700 Hz tone, 5.7 samples a
period (on the choice of the top tones: _pitch_ref.TONES).
"""
import ctypes as C
import os

import numpy as np
import pytest

import _pitch_ref as P
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.analysis import MelAnalyzer

NEW = ["fs2_mel_pitch", "fs2_mel_pitch_lags", "fs2_mel_pitch_tile_frames"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _handle(lib, n_fft=1024, win=1024, hop=256):
    """a handle for the host-side checks: without a device create fails at its upload, after the geometry is in place"""
    basis = np.ones((8, n_fft // 2 + 1), np.float32)
    h = C.c_void_p()
    lib.fs2_mel_create(_lib.FS2_ABI_VERSION, n_fft, win, hop, 8, 1e-6, 0, basis.ctypes.data_as(C.c_void_p), C.byref(h))
    assert h.value
    return h


@pytest.mark.parametrize("name,case", P.CASES)
def test_fragile_frames_stay_within_the_cap(name, case):
    r = P.reference(name, case)
    print(f"{name} / {case}: E_32 = {r['E_32']:.2e}, {r['n_fragile']} of {r['frames']} frames fragile")
    assert 0 < r["E_32"] < 1e-3  # a float32 chain of W terms: far below anything the threshold 0.1 resolves
    assert r["n_fragile"] <= P.MAX_FRAGILE * r["frames"]
    assert len(r["xs"]) <= 12 and r["frames"] == sum(1 + len(x) // P.ALL[name][1] for x in r["xs"])
    if case == "lengths":
        assert [len(x) for x in r["xs"]] == P.seam_lengths(name)


@pytest.mark.parametrize("name", list(P.GEOMETRIES))
def test_definition_finds_the_fundamental_of_noiseless_tones(name):
    win, hop, sr = P.GEOMETRIES[name]
    tau_min, tau_max = P.lags(sr)
    edge = win // hop  # frames whose window or lagged window reaches past the utterance's ends are not interior
    for f in P.TONES[name]:
        x = P.tone(3 * P.TILE[name] * hop, f, sr, 7, noise_db=None)
        tr = P.track(P.cmnd(P.difference64(x, win, hop, tau_max)), sr, tau_min, tau_max)
        inner = tr["f0"][edge:-edge - (tau_max + hop - 1) // hop]
        err = float(np.abs(inner / f - 1.0).max())
        print(f"{name}: {f} Hz, {len(inner)} interior frames, largest relative error {err:.2e}")
        assert len(inner) > 10 and (inner > 0).all() and err <= 0.01, (name, f, err)


@pytest.mark.parametrize("name", list(P.GEOMETRIES))
def test_definition_leaves_noise_and_silence_unvoiced(name):
    win, hop, sr = P.GEOMETRIES[name]
    tau_min, tau_max = P.lags(sr)
    seg = P.TILE[name] * hop // 2 + 11
    x, kinds = P.alternation(seg, P.TONES[name][1], sr, 5)
    cm = P.cmnd(P.difference64(x, win, hop, tau_max))
    tr = P.track(cm, sr, tau_min, tau_max)
    centre = np.arange(len(cm)) * hop
    for i, kind in enumerate(kinds):
        # frames whose window [centre - W / 2, centre + W / 2 + tau_max] lies inside segment i
        inside = (centre - win // 2 >= i * seg) & (centre + win // 2 + tau_max + 1 <= (i + 1) * seg)
        assert inside.sum() >= 2, (name, kind)
        if kind == "voiced":
            assert (np.abs(tr["f0"][inside] / P.TONES[name][1] - 1.0) <= 0.01).all(), (name, i)
        else:
            assert (tr["tau"][inside] == 0).all() and (tr["f0"][inside] == 0).all(), (name, i, kind)
        if kind == "zero":
            assert (cm[inside] == 1.0).all() and (tr["dmin"][inside] == 1.0).all()
    zero = P.track(P.cmnd(P.difference64(np.zeros(5 * hop + 1, np.float32), win, hop, tau_max)), sr, tau_min, tau_max)
    assert (zero["f0"] == 0).all() and (zero["dmin"] == 1.0).all() and len(zero["f0"]) == 6


def test_float32_chain_restates_the_definition():
    """the two restatements agree to float32 rounding on a signal, and exactly where every operation is exact"""
    win, hop, sr = P.GEOMETRIES["small"]
    tau_min, tau_max = P.lags(sr)
    assert (tau_min, tau_max) == (5, 57) and P.lags(22050) == (27, 311)
    x = P.tone(1500, 200.0, sr, 3)
    d64, d32 = P.difference64(x, win, hop, tau_max), P.difference32_chain(x, win, hop, tau_max)
    assert d32.dtype == np.float32 and d64.shape == d32.shape == (1 + 1500 // hop, tau_max + 2)
    assert np.abs(d32 - d64).max() <= 1e-5 * d64.max() and (d64[:, 0] == 0).all()
    ints = np.random.RandomState(0).randint(-8, 9, 900).astype(np.float32)  # small integers: every sum is exact in float32
    assert np.array_equal(P.difference32_chain(ints, win, hop, tau_max).astype(np.float64), P.difference64(ints, win, hop, tau_max))
    one = P.cmnd(P.difference64(np.array([0.5], np.float32), win, hop, tau_max))  # one sample: d(tau) = 2 x^2 for every tau >= 1
    assert one.shape == (1, tau_max + 2) and (one == 1.0).all()


def test_header_declares_the_new_symbols(lib):
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n
    f32, i32 = C.c_float, C.c_int32
    assert lib.fs2_mel_pitch.argtypes == [_lib.DevPtr] * 3 + [i32, i32, i32, f32, f32, f32, _lib.DevPtr, i32] + [_lib.DevPtr] * 3 + [i32, _lib.DevPtr]
    assert lib.fs2_mel_pitch_lags.argtypes[1:4] == [i32, f32, f32] and len(lib.fs2_mel_pitch_lags.argtypes) == 6
    assert lib.fs2_mel_pitch_tile_frames.restype is i32
    assert _lib.FS2_ABI_VERSION == 4  # entry points were only added


def test_lags_tile_and_refusals_on_the_host(lib):
    ARG, SHAPE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_SHAPE
    lo, hi = C.c_int32(-1), C.c_int32(-1)
    for name, (win, hop, sr) in P.ALL.items():
        h = _handle(lib, 1 << (win - 1).bit_length(), win, hop)
        assert lib.fs2_mel_pitch_lags(h, sr, P.F0_FLOOR, P.F0_CEIL, C.byref(lo), C.byref(hi)) == 0
        assert (lo.value, hi.value) == P.lags(sr)
        assert lib.fs2_mel_pitch_tile_frames(h, sr, P.F0_FLOOR) == P.TILE[name]  # the seams the shared cases are placed at
        assert lib.fs2_mel_destroy(h) == 0
    h = _handle(lib)
    msg = lambda: lib.fs2_mel_last_error(h).decode()
    lags = lambda sr, fl, ce: lib.fs2_mel_pitch_lags(h, sr, fl, ce, C.byref(lo), C.byref(hi))
    assert lib.fs2_mel_pitch_lags(None, 22050, 71.0, 800.0, C.byref(lo), C.byref(hi)) == ARG
    assert lib.fs2_mel_pitch_lags(h, 22050, 71.0, 800.0, None, C.byref(hi)) == ARG and "null" in msg()
    lo.value = hi.value = -1
    for (sr, fl, ce), text in (((22050, 21.0, 800.0), "exceeds 1024"), ((22050, 71.0, 70.0), "not below"), ((22050, 71.0, 70.9), "not below"),
                               ((0, 71.0, 800.0), "positive"), ((-5, 71.0, 800.0), "positive"), ((22050, 0.0, 800.0), "positive"),
                               ((22050, -71.0, 800.0), "positive"), ((22050, 71.0, 0.0), "positive"), ((22050, np.nan, 800.0), "positive")):
        assert lags(sr, fl, ce) == SHAPE and text in msg(), (sr, fl, ce, msg())
        if ce == 800.0:  # (the tile does not depend on the ceiling)
            assert lib.fs2_mel_pitch_tile_frames(h, sr, fl) == 0
        # fs2_mel_pitch answers the same, before it looks at any pointer
        assert lib.fs2_mel_pitch(h, None, None, 1, 1, sr, fl, ce, 0.1, None, 1, None, None, None, 0, None) == SHAPE and text in msg()
    assert (lo.value, hi.value) == (-1, -1)  # a refusal writes nothing
    assert lags(22050, 22050 / 1022.0 + 1e-3, 800.0) == 0 and hi.value == 1022  # tau_max + 2 = 1024 is the last that runs
    for thr in (0.0, -0.1, 1.0001, np.nan, np.inf):
        assert lib.fs2_mel_pitch(h, None, None, 1, 1, 22050, 71.0, 800.0, thr, None, 1, None, None, None, 0, None) == SHAPE
        assert "(0, 1]" in msg()
    assert lib.fs2_mel_pitch(None, None, None, 1, 1, 22050, 71.0, 800.0, 0.1, None, 1, None, None, None, 0, None) == ARG
    assert lib.fs2_mel_pitch_tile_frames(None, 22050, 71.0) == 0
    assert lib.fs2_mel_destroy(h) == 0
    h = _handle(lib, 256, 256, 2)  # the span is read in 16-byte words
    assert lib.fs2_mel_pitch_lags(h, 22050, 71.0, 800.0, C.byref(lo), C.byref(hi)) == SHAPE and "multiple of 4" in lib.fs2_mel_last_error(h).decode()
    assert lib.fs2_mel_destroy(h) == 0


def test_items_without_a_contour_still_refuses():
    an = MelAnalyzer.__new__(MelAnalyzer)  # the checks below come before anything touches the device
    an.wada_table = None
    wav, dur = [np.ones(3000, np.float32)], [np.array([3, 4])]
    with pytest.raises(ValueError, match="pitch="):  # the message tests/test_targets_cpu.py matches
        an.items(wav, dur)
    with pytest.raises(ValueError, match="the raw F0 contour per utterance, 0 where unvoiced"):
        an.items(wav, dur, pitch=None)
    with pytest.raises(ValueError, match="'track'"):
        an.items(wav, dur, pitch="yin")
    with pytest.raises(ValueError, match="pitch_options"):
        an.items(wav, dur, pitch=[np.zeros(8, np.float32)], pitch_options={"threshold": 0.2})
