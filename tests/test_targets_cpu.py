"""Training targets without a GPU: the yardsticks of tests/_targets_ref.py (written from include/fs2.h) against what the reference
produced (tests/golden/frontend_targets.npz, tools/gen_golden_targets.py), and what the new entry points refuse before they touch a
device.

The SNR is compared through the MAPPED error |delta out| * (g[i* + 1] - g[i*]): the error carried back to the statistic v3.  The
table's slope varies a hundredfold, so a tolerance in dB would mean nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import _targets_ref as T
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.analysis import MelAnalyzer

NEW = ["fs2_mel_set_snr_table", "fs2_mel_snr", "fs2_op_contour_finish", "fs2_op_masked_row_mean"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def utterances():
    z, meta = T.fixture()
    for case, c in meta["cases"].items():
        for u in range(len(c["utterances"])):
            yield z, meta, c, f"{case}__{u}"


def rel(got, want):
    """|got - want| relative to the row's largest magnitude (a normalised contour crosses zero: an entry-wise ratio means nothing)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)) if got.size else 0.0


def test_wada_yardstick_against_the_reference():
    """Seen here: E_ref = 8.6e-7 over 297 windows (gamma-amplitude "speech" + Gaussian noise at 0-60 dB, 1000-16385 samples, both
    geometries), one window left out as a near-tie."""
    z, meta = T.fixture()
    g = z["wada_table"]
    assert g.shape == (121,) and meta["db_lo"] == -20 and g[3] < g[2], "the reference's table: 121 entries, not monotone at 2 -> 3"
    windows = nan = 0
    for z, meta, c, key in utterances():
        out, v3, idx = T.wada_windows(z[key + "__wav"], c["win_length"], c["hop"], g)
        assert len(out) == len(z[key + "__wada"]) == -(-len(z[key + "__wav"]) // c["hop"])
        windows, nan = windows + len(out), nan + int(np.isnan(out).sum())
    E = T.e_ref()
    print(f"E_ref = {E:.2e} over {windows} windows, {nan} of them NaN")
    assert windows > 200 and nan > 0
    assert 0 < E < T.E_REF_BOUND


def test_wada_lookup_edges():
    g = np.array([0.5, 0.6, 0.55, 0.7, 0.9])  # not monotone: the LARGEST index below v3 counts
    assert T.wada_lookup(0.58, g) == (pytest.approx(2 + 0.03 / 0.15), 2)
    assert np.isnan(T.wada_lookup(0.5, g)[0]) and np.isnan(T.wada_lookup(0.2, g)[0])  # nothing strictly below
    assert np.isnan(T.wada_lookup(0.95, g)[0]) and np.isnan(T.wada_lookup(np.inf, g)[0]) and np.isnan(T.wada_lookup(np.nan, g)[0])
    assert np.isnan(T.wada_lookup(0.9, g)[0])  # i* = 3, out = 4 = K - 1: NaN unless out < K - 1
    x = np.zeros(600, np.float32)
    x[300:] = np.random.RandomState(0).standard_normal(300)
    out, v3, idx = T.wada_windows(x, 256, 64, g)
    assert len(out) == 10 and np.isnan(out[0]) and np.isnan(v3[0])  # a window of exact zeros
    assert np.isnan(T.wada_windows(np.full(300, 0.25, np.float32), 256, 64, g)[0]).all()  # constant: v3 = 0, below the table


def test_finishing_and_priors_yardsticks_against_the_reference():
    for z, meta, c, key in utterances():
        d, sil = z[key + "__duration"], z[key + "__silent"]
        fsil = z[key + "__silence_mask"]
        assert np.array_equal(T.expand(sil, d), fsil)
        assert all(int(d[:j].sum()) >= j for j in range(len(d))), "the in-place phone means read original frames only"
        for tag, kw in (("raw", {}), ("stats", meta["stats"]["snr"])):
            y, F, prior = T.finish(z[key + "__wada"], d, sil, None, False, 0.0, **kw)
            want = z[f"{key}__frame__{tag}__snr"]
            assert F == len(want) == int(d.sum()) and (y[F:] == 0).all()
            assert rel(y[:F], want) <= 1e-6, (key, tag)
            if tag == "raw" and key + "__prior_snr" in z.files:
                assert abs(prior - float(z[key + "__prior_snr"])) <= 1e-6 * abs(float(z[key + "__prior_snr"]))
                assert abs(T.prior(want, fsil) - float(z[key + "__prior_snr"])) <= 1e-6 * abs(float(z[key + "__prior_snr"]))
                assert abs(T.prior(z[f"{key}__frame__raw__energy"], fsil) - float(z[key + "__prior_energy"])) <= 1e-6 * float(z[key + "__prior_energy"])
        if sil.all():
            assert (z[f"{key}__frame__raw__snr"] == 0).all() and np.isnan(T.finish(z[key + "__wada"], d, sil)[2])
        else:
            assert abs(T.prior(d, sil) - float(z[key + "__prior_duration"])) <= 1e-6 * float(z[key + "__prior_duration"])
        y, F, prior = T.finish(z[key + "__f0"], d, sil, None, True, 1e-7)
        assert F == len(z[key + "__pitch"]) and rel(y[:F], z[key + "__pitch"]) <= 1e-6, key
        # phone level: every phone averages the finished frames, 1e-7 for an empty one, then the stats
        fin = T.finish(z[key + "__wada"], d, sil)[0]
        pos = np.concatenate([[0], np.cumsum(d)])
        st = meta["stats"]["snr"]
        phone = np.array([fin[pos[j]:pos[j + 1]].mean() if d[j] > 0 else 1e-7 for j in range(len(d))])
        assert rel(phone, z[f"{key}__phone__raw__snr"]) <= 1e-6
        assert rel((phone - st["mean"]) / st["std"], z[f"{key}__phone__stats__snr"]) <= 1e-6


def test_finish_yardstick_cases():
    nan = np.nan
    y, F, p = T.finish([nan, 2.0, nan, nan, 8.0, nan, 5.0], [2, 0, 3, -4, 1], silent=[0, 1, 0, 0, 1], frames=7)
    assert F == 6 and np.allclose(y, [2, 2, 4, 6, 8, 8, 0]) and p == pytest.approx(np.mean([2, 2, 4, 6, 8]))
    y, F, p = T.finish([0.0, 3.0, 0.0], [3], zero_is_missing=True)
    assert np.allclose(y, [3, 3, 3])
    y, F, p = T.finish([0.0, 3.0, 0.0], [3], zero_is_missing=False, mean=1.0, std=2.0)
    assert np.allclose(y, [-0.5, 1.0, -0.5]) and p == 1.0
    y, F, p = T.finish([0.0, 0.0, 5.0], [2, 9], zero_is_missing=True, all_missing_value=1e-7, frames=2)
    assert F == 2 and np.allclose(y, [1e-7, 1e-7, 0]) and p == pytest.approx(1e-7)


# ---- the C ABI, no device
def _handle(lib, n_fft=1024, win=1024, hop=256):
    basis = np.ones((80, n_fft // 2 + 1), np.float32)
    h = C.c_void_p()
    st = lib.fs2_mel_create(_lib.FS2_ABI_VERSION, n_fft, win, hop, 80, 1e-6, 0, basis.ctypes.data_as(C.c_void_p), C.byref(h))
    assert h.value
    return st, h


def test_snr_table_and_snr_refuse_bad_arguments(lib):
    ARG, STATE, SHAPE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_STATE, _lib.FS2_ERR_SHAPE
    st, h = _handle(lib)
    good = np.linspace(0.4, 1.6, 121)
    bad = good.copy()
    bad[60] = np.nan
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = lib.fs2_mel_set_snr_table
    assert f(None, p(good), 121, -20) == ARG
    for args, text in (((None, 121), "null"), ((p(good), 1), "entries"), ((p(good), 513), "entries"), ((p(bad), 121), "not finite")):
        assert f(h, args[0], args[1], -20) == ARG and text in lib.fs2_mel_last_error(h).decode(), args
    assert f(h, p(good), 121, np.inf) == ARG
    # no table yet (and, without a device, no handle that could take one): FS2_ERR_STATE, nothing read
    assert lib.fs2_mel_snr(h, None, None, 1, 1, 1, None, 1, None, None, 0, None) == STATE
    assert lib.fs2_mel_snr(None, None, None, 1, 1, 1, None, 1, None, None, 0, None) == ARG
    if st == _lib.FS2_OK:  # with a device the handle is good: the message names the missing table
        assert "fs2_mel_set_snr_table" in lib.fs2_mel_last_error(h).decode()
    assert lib.fs2_mel_destroy(h) == 0
    # win_length must be a multiple of hop.  (1024 / 768 / 256 is fine - 768 = 3 * 256: three hops per window; 1024 / 768 / 512 and
    # 1024 / 800 / 256 are not.)
    for (n_fft, win, hop), want_shape in (((1024, 768, 512), True), ((1024, 800, 256), True), ((1024, 768, 256), False)):
        st, h = _handle(lib, n_fft, win, hop)
        got = lib.fs2_mel_snr(h, None, None, 1, 1, 1, None, 1, None, None, 0, None)
        assert (got == SHAPE) == want_shape and got != 0, (n_fft, win, hop, got)
        if want_shape:
            assert "multiple of hop" in lib.fs2_mel_last_error(h).decode()
        assert lib.fs2_mel_destroy(h) == 0
    st, h = _handle(lib, 1000, 1000, 250)  # a handle whose geometry create refused has none to judge
    assert st == SHAPE and lib.fs2_mel_snr(h, None, None, 1, 1, 1, None, 1, None, None, 0, None) == STATE
    assert lib.fs2_mel_destroy(h) == 0


def test_contour_finish_and_row_mean_refuse_bad_arguments(lib):
    ARG, SHAPE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_SHAPE
    v, d, o, fo = (C.c_float * 8)(), (C.c_int32 * 8)(), (C.c_float * 8)(), (C.c_int32 * 8)()
    f = lib.fs2_op_contour_finish

    def call(values=v, dur=d, out=o, fout=fo, B=1, T=8, L=8, mean=0.0, std=1.0):
        return f(values, None, dur, None, B, T, L, 0, 0, mean, std, out, fout, None, None)
    assert call(std=0.0) == ARG and call(std=np.nan) == ARG and call(std=np.inf) == ARG and call(mean=np.nan) == ARG
    assert call(values=None) == ARG and call(dur=None) == ARG and call(out=None) == ARG and call(fout=None) == ARG
    assert call(B=0) == ARG and call(T=0) == ARG and call(L=0) == ARG
    assert call(T=4097) == SHAPE and call(L=2049) == SHAPE  # the documented limits: 4096 frames, 2048 phones
    g = lib.fs2_op_masked_row_mean
    assert g(None, None, None, 1, 8, o, None) == ARG and g(v, None, None, 1, 8, None, None) == ARG
    assert g(v, None, None, 0, 8, o, None) == ARG and g(v, None, None, 1, 0, o, None) == ARG


def test_new_symbols_and_python_surface(lib):
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n), n
    assert lib.fs2_mel_set_snr_table.argtypes == [_lib.DevPtr, _lib.DevPtr, C.c_int32, C.c_float]
    assert len(lib.fs2_mel_snr.argtypes) == 12 and lib.fs2_mel_snr.argtypes[10] is C.c_size_t
    assert lib.fs2_op_contour_finish.argtypes[7:11] == [C.c_int32, C.c_float, C.c_float, C.c_float] and len(lib.fs2_op_contour_finish.argtypes) == 15
    assert len(lib.fs2_op_masked_row_mean.argtypes) == 7
    assert _lib.FS2_ABI_VERSION == 4  # entry points were only added
    import lightningfastspeech2_amd as pkg
    assert pkg.finish_contour.__name__ == "finish_contour" and pkg.masked_row_mean.__name__ == "masked_row_mean"
    an = MelAnalyzer.__new__(MelAnalyzer)  # the checks below come before anything touches the device
    an.wada_table = None
    wav, dur = [np.ones(3000, np.float32)], [np.array([3, 4])]
    with pytest.raises(ValueError, match="pitch="):
        an.items(wav, dur)
    with pytest.raises(ValueError, match="prior 'snr'"):
        an.items(wav, dur, variances=("energy",), levels=("frame",), priors=("snr",))
    with pytest.raises(ValueError, match="levels"):
        an.items(wav, dur, variances=("energy",), levels=("frame", "phone"))
    with pytest.raises(ValueError, match="none of"):
        an.items(wav, dur, variances=("srmr",), levels=("frame",))
    with pytest.raises(RuntimeError, match="wada_values.npy"):
        an.snr(wav)
