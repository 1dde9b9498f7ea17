"""The CWT variance transform's restatement (tests/_cwt_ref.py) - the yardstick tests/test_gpu_cwt.py holds the device to - checked
without a GPU: closed forms of ``ricker`` / ``cwt`` (SciPy 1.14's definition; SciPy 1.15 removed both, so there is nothing to run
them against), ``decompose_ref`` against the reference's own ``CWT.decompose`` where that tree is present, and the checks
``MelAnalyzer.items`` makes of its ``transforms`` argument before it touches the device."""
import importlib.util
import math
import os

import numpy as np
import pytest

import _cwt_ref as R
from tools.ref_import import REFERENCE_ROOT

REFERENCE_CWT = os.path.join(REFERENCE_ROOT, "litfass", "dataset", "cwt.py")


def _formula(v, w):
    return 2.0 / (math.sqrt(3.0 * w) * math.pi ** 0.25) * (1.0 - v * v / (w * w)) * math.exp(-v * v / (2.0 * w * w))


def test_ricker_at_hand_computed_points():
    w = 4 * R.TAU  # scale 1
    r = R.ricker(12, w)
    assert r.shape == (12,) and r.dtype == np.float64
    for m in (0, 3, 5, 6, 11):  # v = m - 5.5
        assert r[m] == pytest.approx(_formula(m - 5.5, w), rel=1e-14, abs=1e-300)
    assert np.array_equal(r, r[::-1])  # an integer point count is symmetric
    # a = 2, 11 points: the middle sample is the amplitude 2 / (sqrt(6) pi^(1/4)) = 2 / (2.4494897 * 1.3313354) = 2 / 3.2610923 = 0.6132914
    assert R.ricker(11, 2.0)[5] == pytest.approx(0.6132914, abs=1e-6)
    # the zero crossings lie at v = +- a: 12 points, a = 2.5 -> v = m - 5.5 = 2.5 at m = 8 (and -2.5 at m = 3)
    z = R.ricker(12, 2.5)
    assert z[8] == 0.0 and z[3] == 0.0 and z[7] > 0 > z[9]
    # one sample: v = 0
    assert R.ricker(1, 3.0).tolist() == [pytest.approx(2.0 / (3.0 * math.pi ** 0.25))]


def test_untruncated_scale_1_has_12_points_about_5_1667():
    w = R.widths()[0]
    assert w == 4 * R.TAU and 10 * w == pytest.approx(11.3337)
    r = R.ricker(10 * w, w)
    centre = (10 * w - 1.0) / 2
    assert len(r) == 12 and centre == pytest.approx(5.16685, abs=1e-6)
    for m in range(12):
        assert r[m] == pytest.approx(_formula(m - centre, w), rel=1e-13, abs=1e-300)
    assert r[5] > r[6] and not np.array_equal(r, r[::-1])  # not symmetric about the middle sample
    # every untruncated scale: ceil(10 w) points
    assert [len(R.ricker(10 * x, x)) for x in R.widths()] == [12, 23, 46, 91, 182, 363, 726, 1451, 2902, 5803]


@pytest.mark.parametrize("n, p", [(200, 77), (201, 100), (13, 0), (13, 12), (12, 5)])
def test_an_impulse_returns_the_reversed_wavelet_at_the_right_offset(n, p):
    """data = delta at p: c[k] = r[M - 1 - (k + (M - 1) // 2 - p)], i.e. the reversed wavelet with its sample t at k = p - (M - 1) // 2 + t,
    cut at the ends - for even and odd M, truncated (M = n) and not"""
    data = np.zeros(n, np.float32)
    data[p] = 1.0
    ws = R.widths()
    out = R.cwt(data, R.ricker, ws)
    parities = set()
    for i, w in enumerate(ws):
        r = R.ricker(min(10 * w, n), w)
        M = len(r)
        assert M == math.ceil(min(10 * w, n))
        parities.add((M % 2, M == n))
        want = np.zeros(n)
        for t in range(M):
            k = p - (M - 1) // 2 + t
            if 0 <= k < n:
                want[k] = r[M - 1 - t]
        assert np.array_equal(out[i], want), (i, M)
    if n >= 200:
        assert {(0, False), (1, False)} <= parities and (n % 2, True) in parities


def test_decompose_dtypes_and_exact_cases():
    v = R.contour(50, 1)
    v[7] = 0.0
    ref, f64 = R.decompose_ref(v), R.decompose_f64(v)
    assert ref["signal"].dtype == np.float32 and ref["original_signal"].dtype == np.float32 and ref["mean"].dtype == np.float32
    assert ref["spectrogram"].shape == (50, 10) and ref["spectrogram"].dtype == np.float64
    assert f64["signal"].dtype == np.float64 and f64["mean"].dtype == np.float64
    assert ref["original_signal"][7] == np.float32(1e-7) and f64["original_signal"][7] == float(np.float32(1e-7))
    assert v[7] == 0.0  # the caller's array is not written
    assert np.abs(ref["spectrogram"] - f64["spectrogram"]).max() < 1e-5 * np.abs(f64["spectrogram"]).max()
    const = R.decompose_f64(np.full(40, 123.0, np.float32))
    assert const["std"] == 0.0 and not const["spectrogram"].any()
    one = R.decompose_ref(np.array([200.0], np.float32))
    assert one["std"] == 0.0 and one["spectrogram"].shape == (1, 10) and not one["spectrogram"].any()


@pytest.mark.skipif(not os.path.exists(REFERENCE_CWT), reason="the reference tree is not here")
def test_decompose_ref_is_the_references_decompose_bit_for_bit():
    """The reference's own dataset/cwt.py, loaded from its path under a private name with this restatement's cwt / ricker standing
    in for the two functions SciPy removed: widths, constants, the transpose, the zero replacement and the dtype order are then the
    reference's text, and only the convolution is ours."""
    scipy_signal = pytest.importorskip("scipy.signal")
    missing = object()
    before = {n: getattr(scipy_signal, n, missing) for n in ("cwt", "ricker")}
    try:
        scipy_signal.cwt, scipy_signal.ricker = R.cwt, R.ricker
        spec = importlib.util.spec_from_file_location("_fs2_reference_dataset_cwt", REFERENCE_CWT)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, val in before.items():  # (tools/ref_import.py may have set them to None: that is put back too)
            if val is missing:
                delattr(scipy_signal, n)
            else:
                setattr(scipy_signal, n, val)
    obj = mod.CWT()
    assert (obj.n_scales, obj.tau) == (R.N_SCALES, R.TAU)
    rows = [R.contour(n, 40 + n) for n in (1, 2, 12, 47, 200, 365, 800)]
    rows[3][[0, 20]] = 0.0
    rows[5][364] = 0.0
    for v in rows:
        got, want = obj.decompose(v.copy()), R.decompose_ref(v)
        assert sorted(got) == sorted(want) == ["mean", "original_signal", "signal", "spectrogram", "std"]
        for k in want:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (len(v), k)


def test_items_refuses_an_unknown_transform_before_the_device():
    from lightningfastspeech2_amd.analysis import MelAnalyzer
    an = MelAnalyzer.__new__(MelAnalyzer)  # the checks below come before anything touches the device
    an.wada_table = None
    wav, dur = [np.ones(3000, np.float32)], [np.array([3, 4])]
    f0 = [np.full(12, 100.0, np.float32)]
    with pytest.raises(ValueError, match="transforms must name one of"):
        an.items(wav, dur, pitch=f0, transforms=("cwt", "wavelet", "none"))
    with pytest.raises(ValueError, match="transforms must name one of"):
        an.items(wav, dur, pitch=f0, transforms=("cwt",))  # one per variance
    with pytest.raises(ValueError, match="transforms must name one of"):
        an.items(wav, dur, variances=("energy",), levels=("frame",), transforms=("CWT",))
    with pytest.raises(ValueError, match="pitch="):  # a valid list passes on to the next check
        an.items(wav, dur, transforms=("cwt", "none", "log"))
