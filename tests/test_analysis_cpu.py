"""The analysis front end without a GPU: the Slaney basis from its definition, the CPU yardsticks of tests/_analysis_ref.py against
an explicit DFT and against each other, and what fs2_mel_create refuses before it touches a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _analysis_ref as R
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.analysis import slaney_mel_basis, slaney_mel_edges

SIGNALS = ("noise", "ramp", "tone440", "tone3k")
N_SAMPLES = 24000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- the basis
def test_basis_shape_sign_and_single_peak():
    for sr, n_fft, n_mels, fmin, fmax in ((22050, 1024, 80, 0, 8000), (16000, 512, 40, 50, None), (22050, 256, 20, 0, 8000)):
        b = slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax)
        assert b.shape == (n_mels, n_fft // 2 + 1) and b.dtype == np.float32
        assert (b >= 0).all() and np.isfinite(b).all()
        for row in b:
            nz = np.nonzero(row)[0]
            if len(nz) == 0:
                continue  # a band narrower than a bin spacing may fall between two bins
            assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))  # one run of non-zeros ...
            k = int(row.argmax())
            assert (np.diff(row[nz[0]:k + 1]) >= 0).all() and (np.diff(row[k:nz[-1] + 1]) <= 0).all()  # ... rising, then falling


def test_basis_support_and_area():
    sr, n_fft, n_mels = 22050, 1024, 80
    b = slaney_mel_basis(sr, n_fft, n_mels, 0, 8000).astype(np.float64)
    edges = slaney_mel_edges(n_mels, 0, 8000)
    freqs = np.arange(n_fft // 2 + 1) * sr / n_fft
    for m in range(n_mels):
        inside = (freqs > edges[m]) & (freqs < edges[m + 2])
        assert (b[m][~inside] == 0).all() and (b[m][inside] > 0).all(), m
        assert b[m].max() <= 2.0 / (edges[m + 2] - edges[m]) * (1 + 1e-6)
    # the continuous triangle of height 2 / (f[m+2] - f[m]) has unit area in Hz: on a fine bin grid the Riemann sum shows it
    fine = slaney_mel_basis(sr, 1 << 16, n_mels, 0, 8000).astype(np.float64)
    area = fine.sum(axis=1) * sr / (1 << 16)
    assert np.abs(area - 1.0).max() < 1e-3


def test_slaney_scale_breakpoints():
    # linear at 200/3 Hz per mel below 1 kHz: 15 mel = 1 kHz; above it 27 steps per factor 6.4: 42 mel = 6.4 kHz
    edges = slaney_mel_edges(40, 0.0, 6400.0)  # 42 mel over 41 intervals
    mel = np.linspace(0.0, 42.0, 42)
    low = mel <= 15.0
    assert np.allclose(edges[low], mel[low] * 200.0 / 3.0, rtol=1e-12)
    assert np.allclose(edges[~low], 1000.0 * 6.4 ** ((mel[~low] - 15.0) / 27.0), rtol=1e-12)
    assert edges[0] == 0.0 and abs(edges[-1] - 6400.0) < 1e-9
    e2 = slaney_mel_edges(13, 0.0, 1000.0)  # entirely in the linear part: equally spaced in Hz
    assert np.allclose(np.diff(e2), 1000.0 / 14.0, rtol=1e-12)


def test_default_basis_weighs_bins_1_to_371_only():
    b = slaney_mel_basis()
    assert b.shape == (80, 513)
    assert (b[:, 0] == 0).all() and (b[:, 372:] == 0).all()
    used = np.nonzero(b.any(axis=0))[0]
    assert used[0] == 1 and used[-1] == 371 and len(used) == 371


# ---- the yardsticks
def test_float64_reference_is_the_dft_of_the_stated_frames():
    rng = np.random.RandomState(1)
    for win in (16, 12):
        g = R.Geometry(n_fft=16, win_length=win, hop=4, n_mels=3)
        x = rng.standard_normal(50).astype(np.float32)
        fr = R.frames_of(x.astype(np.float64), g)
        w = np.zeros(16)
        w[(16 - win) // 2:(16 - win) // 2 + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
        want = np.zeros((fr.shape[0], 9))
        for t in range(fr.shape[0]):
            for f in range(9):  # the O(N^2) DFT, term by term
                acc = 0j
                for k in range(16):
                    acc += w[k] * fr[t, k] * np.exp(-2j * np.pi * f * k / 16)
                want[t, f] = abs(acc)
        got = R.stft_mag(torch.from_numpy(x).double(), g, torch.float64).numpy()
        assert got.shape == want.shape == (1 + 50 // 4, 9)
        assert np.abs(got - want).max() < 1e-12
        cos64, sin64 = R.dft_tables(g)  # the chain model's tables are that DFT too
        assert np.abs(np.hypot(fr @ cos64, fr @ sin64) - want).max() < 1e-12


def test_frame_counts_at_the_short_end():
    g = R.Geometry()
    basis = slaney_mel_basis()
    for n in (1, g.hop - 1, g.hop, g.hop + 1, g.n_fft // 2 - 1):
        x = R.signal("noise", n, seed=n)
        T, Te = R.frame_counts(n, g.hop)
        assert (T, Te) == (1 + n // g.hop, (n + g.hop - 1) // g.hop)
        assert R.mel_ref(x, g, basis).shape == (T, 80) and R.mel_chain(x, g, basis).shape == (T, 80)
        assert R.energy_ref(x, g).shape == (Te,) and R.energy_chain(x, g).shape == (Te,)


@pytest.mark.parametrize("kind", SIGNALS)
def test_float32_recipe_and_chain_model_against_float64(kind):
    """Seen here (24,000 samples at 22.05 kHz, seed 0, no peak normalisation): linear figure of the fp32 recipe 1.6-2.2e-7 (the
    operator's specification quotes 1.2-2.3e-7), of the chain model 6.4-9.1e-7 (4.9-9.2e-7); log10 error of the chain model at the kept entries
    6.6e-7 on noise and 9.5e-7 on the ramp, every entry kept (<= 5.8e-7), 1.46e-5 on the 440 Hz tone and 6.8e-6 on the 3 kHz tone
    (<= 1.1e-5).  The asserts are 1.2x what was seen; the chain model's linear bound is the specified 1.5e-6.
    The log selection keeps 13.5 % (440 Hz) and 8.2 % (3 kHz) of the tone entries, not the specification's 23-24 %: the share is the
    fraction of a frame's 80 bands within three decades of its peak band, which depends on how far the signal's leakage and noise
    floor reach - on the tone's length, phase and noise seed and on the basis' normalisation, none of which it states; its
    chain model also rounds differently (its figures suggest fused multiply-adds, this one rounds product and sum separately)."""
    g = R.Geometry()
    basis = slaney_mel_basis()
    x = R.signal(kind, N_SAMPLES)
    m64 = R.mel_ref(x, g, basis, peak_normalize=False)
    m32 = R.mel_ref(x, g, basis, peak_normalize=False, dtype=torch.float32)
    mc = R.mel_chain(x, g, basis, peak_normalize=False)
    lin_b, lin_c = R.linear_figure(m32, m64), R.linear_figure(mc, m64)
    log_c, keep = R.log_figure(R.log10_f32(mc, g.clip), m64, g.clip)
    print(f"{kind}: linear fp32 recipe {lin_b:.2e}, chain {lin_c:.2e}; log10 chain {log_c:.2e} at {keep:.3f} of the entries")
    log_bar, keep_want = {"noise": (8e-7, 1.0), "ramp": (1.15e-6, 1.0), "tone440": (1.75e-5, 0.135), "tone3k": (8.2e-6, 0.082)}[kind]
    assert lin_b <= 2.6e-7
    assert lin_b < lin_c <= 1.5e-6  # the yardstick cannot drift
    assert log_c <= log_bar
    assert keep == 1.0 if keep_want == 1.0 else abs(keep - keep_want) <= 0.005


def test_energy_and_segment_mean_models():
    g = R.Geometry()
    x = R.signal("noise", 3000, seed=5)
    e64, e32 = R.energy_ref(x, g), R.energy_chain(x, g)
    assert e64.shape == e32.shape == (12,) and np.abs(e32 / e64 - 1).max() < 1e-5
    xs = x.astype(np.float64) / np.abs(x).max()
    assert abs(e64[11] - np.sqrt(np.sum(xs[11 * 256:] ** 2) / 1024)) < 1e-15  # truncated at the end, divided by the full window
    v = np.arange(10, dtype=np.float64)
    got = R.segment_mean_ref(v, 8, [2, 0, 3, 5, 4], mean=1.0, std=2.0)
    assert np.allclose(got, [(0.5 - 1) / 2, (1e-7 - 1) / 2, (3.0 - 1) / 2, (6.0 - 1) / 2, (1e-7 - 1) / 2])  # clipped at 8; empty past it


# ---- the C ABI, no device
def _create(lib, n_fft=1024, win=1024, hop=256, n_mels=80, clip=1e-6, kind=0, basis="default", abi=None):
    if isinstance(basis, str):
        basis = np.ascontiguousarray(np.abs(np.random.RandomState(0).standard_normal((max(n_mels, 1), n_fft // 2 + 1))), np.float32)
    h = C.c_void_p()
    st = lib.fs2_mel_create(_lib.FS2_ABI_VERSION if abi is None else abi, n_fft, win, hop, n_mels, clip, kind,
                            None if basis is None else basis.ctypes.data_as(C.c_void_p), C.byref(h))
    msg = lib.fs2_mel_last_error(h).decode()
    assert h.value, "the handle comes back on failure too"
    ws = lib.fs2_mel_ws_bytes(h, 4, 1000)
    run = lib.fs2_mel_run(h, None, None, 1, 1, 0, None, 1, None, 1, None, None, None, 0, None)
    assert lib.fs2_mel_destroy(h) == 0
    return st, msg, ws, run


def test_mel_create_refuses_bad_configs_before_any_device_call(lib):
    ARG, SHAPE, STATE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_SHAPE, _lib.FS2_ERR_STATE
    nan_basis = np.ones((80, 513), np.float32)
    nan_basis[40, 200] = np.nan
    inf_basis = np.ones((80, 513), np.float32)
    inf_basis[0, 0] = np.inf
    cases = [
        (dict(abi=_lib.FS2_ABI_VERSION + 1), ARG, "abi_version"),
        (dict(n_fft=1000), SHAPE, "n_fft 1000"),
        (dict(n_fft=128, win=128, hop=32), SHAPE, "n_fft 128"),
        (dict(n_fft=4096), SHAPE, "n_fft 4096"),
        (dict(win=1025), SHAPE, "win_length 1025"),
        (dict(win=0), SHAPE, "win_length 0"),
        (dict(hop=300), SHAPE, "hop 300"),
        (dict(hop=0), SHAPE, "hop 0"),
        (dict(n_mels=0), SHAPE, "n_mels 0"),
        (dict(n_mels=129), SHAPE, "n_mels 129"),
        (dict(basis=None), ARG, "null"),
        (dict(basis=nan_basis), ARG, "not finite"),
        (dict(basis=inf_basis), ARG, "not finite"),
        (dict(clip=0.0), ARG, "clip"),
        (dict(kind=3), ARG, "log_kind"),
    ]
    for kw, want, text in cases:
        st, msg, ws, run = _create(lib, **kw)
        assert st == want and text in msg, (kw, st, msg)
        assert run == STATE, kw  # a handle whose create failed runs nothing
    assert lib.fs2_mel_create(_lib.FS2_ABI_VERSION, 1024, 1024, 256, 80, 1e-6, 0, nan_basis.ctypes.data_as(C.c_void_p), None) == ARG
    assert lib.fs2_mel_destroy(None) == ARG and lib.fs2_mel_last_error(None) == b"null mel handle"
    assert lib.fs2_mel_ws_bytes(None, 4, 1000) == 0 and lib.fs2_mel_tile_frames(None) == 0
    if not torch.cuda.is_available():  # a good config gets as far as the device, and says so
        st, msg, ws, run = _create(lib)
        assert st == _lib.FS2_ERR_HIP and "hipMalloc" in msg and run == STATE and ws == 256


def test_segment_mean_refuses_bad_arguments(lib):
    one = (C.c_float * 4)()
    d = (C.c_int32 * 4)()
    f = lib.fs2_op_segment_mean
    assert f(None, None, d, 1, 4, 4, 1e-7, 0, 1, one, None) == _lib.FS2_ERR_ARG
    assert f(one, None, None, 1, 4, 4, 1e-7, 0, 1, one, None) == _lib.FS2_ERR_ARG
    assert f(one, None, d, 1, 4, 4, 1e-7, 0, 1, None, None) == _lib.FS2_ERR_ARG
    assert f(one, None, d, 0, 4, 4, 1e-7, 0, 1, one, None) == _lib.FS2_ERR_ARG
    assert f(one, None, d, 1, 4, 4, 1e-7, 0, 0, one, None) == _lib.FS2_ERR_ARG  # std 0
    assert f(one, None, d, 1, 4, 4, 1e-7, 0, np.nan, one, None) == _lib.FS2_ERR_ARG


def test_declared_symbols_and_types(lib):
    names = _lib.declared_symbols()
    new = ["fs2_mel_create", "fs2_mel_destroy", "fs2_mel_last_error", "fs2_mel_tile_frames", "fs2_mel_used_bins", "fs2_mel_ws_bytes",
           "fs2_mel_run", "fs2_op_segment_mean"]
    for n in new:
        assert n in names and hasattr(lib, n), n
    assert (_lib.FS2_MEL_LOG10, _lib.FS2_MEL_LN, _lib.FS2_MEL_LINEAR) == (0, 1, 2)
    assert lib.fs2_mel_create.argtypes == [C.c_int32] * 5 + [C.c_float, C.c_int32, _lib.DevPtr, C.POINTER(C.c_void_p)]
    assert lib.fs2_mel_ws_bytes.restype is C.c_size_t and lib.fs2_mel_last_error.restype is C.c_char_p
    assert lib.fs2_mel_run.argtypes[13] is C.c_size_t and len(lib.fs2_mel_run.argtypes) == 15
    assert lib.fs2_op_segment_mean.argtypes[6:9] == [C.c_float] * 3


def test_python_surface_without_a_gpu():
    import lightningfastspeech2_amd as pkg
    assert pkg.slaney_mel_basis is slaney_mel_basis and pkg.MelAnalyzer.__name__ == "MelAnalyzer"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.MelAnalyzer(device="cpu")
    with pytest.raises(ValueError, match="fmin"):
        slaney_mel_basis(22050, 1024, 80, 0, 20000)
