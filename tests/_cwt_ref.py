"""Test helper (CPU): the CWT variance transform restated - ``scipy.signal.ricker`` and ``scipy.signal.cwt`` from the definition
SciPy 1.14 published (both were removed in 1.15), and ``CWT.decompose`` (litfass/dataset/cwt.py:30-46) on top of them.

Not pinned against SciPy's output (its ``cwt`` is gone).  tests/test_cwt_cpu.py holds ``ricker`` / ``cwt`` to closed forms and, where
the reference tree is present, ``decompose_ref`` to the reference's own ``CWT.decompose`` bit for bit.

``decompose_ref`` keeps the reference's dtype order (float32 log, numpy's float32 mean / std, a float32 normalised signal, the
convolution in float64); ``decompose_f64`` is the same definition in float64 throughout - the truth an error is measured against."""
import functools

import numpy as np

N_SCALES, TAU = 10, 0.2833425
EPS = np.float32(1e-7)  # the zero replacement and the std guard: both float32 in the reference (a float32 array takes the scalar)

# lengths around every scale's truncation point 10 w (11.33, 22.67, 45.3, 90.7, 181.3, 362.7, 725.4, 1450.7, 2901.4), both parities of
# M, the device kernel's output tiles (512) and wavefronts, and the cap
COUNTS = (1, 2, 3, 11, 12, 13, 22, 23, 24, 45, 46, 63, 64, 65, 90, 91, 181, 182, 255, 256, 257, 362, 363, 364, 725, 726, 1450, 1451, 1452,
          1536, 2901, 2902, 4095, 4096)
ZERO_ROWS = (3, 12, 64, 363, 1536, 4096)  # counts whose rows get a few exact zeros


def ricker(points, a):
    """The Ricker ("Mexican hat") wavelet as SciPy 1.14 defines it: ceil(points) samples of
    A (1 - v^2 / a^2) exp(-v^2 / (2 a^2)),  v = m - (points - 1) / 2,  A = 2 / (sqrt(3 a) pi^(1/4)).
    `points` may be a real number (cwt passes min(10 a, len(data))): the sample count is then ceil(points) while the centre stays
    (points - 1) / 2, so the samples are not symmetric about the middle one."""
    A = 2 / (np.sqrt(3 * a) * (np.pi ** 0.25))
    wsq = a ** 2
    vec = np.arange(0, points) - (points - 1.0) / 2
    xsq = vec ** 2
    return A * (1 - xsq / wsq) * np.exp(-xsq / (2 * wsq))


def same_convolve(data, kernel):
    """``scipy.signal.convolve(data, kernel, mode="same")``: the full convolution, then the len(data) outputs centred in it (the
    slice starts at (len(full) - len(data)) // 2 = (len(kernel) - 1) // 2)"""
    full = np.convolve(data, kernel)  # mode "full", the direct sum; float32 data times a float64 kernel is float64
    start = (len(full) - len(data)) // 2
    return full[start:start + len(data)]


def cwt(data, wavelet, widths):
    """(len(widths), len(data)) float64: per width w the `same` convolution of data with wavelet(min(10 w, len(data)), w) reversed"""
    out = np.empty((len(widths), len(data)), np.float64)
    for i, w in enumerate(widths):
        n_points = np.min([10 * w, len(data)])
        out[i] = same_convolve(data, wavelet(n_points, w)[::-1])
    return out


def widths(n_scales=N_SCALES, tau=TAU):
    return [2 ** (i + 1) * tau for i in range(1, n_scales + 1)]


def gains(n_scales=N_SCALES):
    return np.array([(i + 2.5) ** (-5 / 2) for i in range(1, n_scales + 1)])


def _decompose(values, dtype, n_scales, tau):
    signal = np.array(values, np.float32).astype(dtype)
    signal[signal == 0] = EPS
    original = signal.copy()
    with np.errstate(invalid="ignore"):
        signal = np.log(signal)
    x = (signal - signal.mean()) / (signal.std() + EPS.astype(dtype))
    spec = cwt(x, ricker, widths(n_scales, tau)) * gains(n_scales)[:, None]
    return {"signal": signal, "original_signal": original, "spectrogram": spec.T, "mean": signal.mean(), "std": signal.std()}


def decompose_ref(values, n_scales=N_SCALES, tau=TAU):
    """``CWT.decompose`` in the reference's dtype order: `values` is float32, and so are the log, numpy's mean and std and the
    normalised signal; the convolution is float64"""
    return _decompose(values, np.float32, n_scales, tau)


def decompose_f64(values, n_scales=N_SCALES, tau=TAU):
    """the same definition on the same float32 input, float64 everywhere"""
    return _decompose(values, np.float64, n_scales, tau)


def contour(n, seed):
    """n positive float32 values shaped like an F0 contour: log-normal about 180 Hz, smooth, clipped to 80 .. 400 Hz"""
    rs = np.random.RandomState(seed)
    walk = np.cumsum(rs.standard_normal(n)) * 0.03
    walk -= walk.mean()
    return np.clip(180.0 * np.exp(0.35 * np.sin(np.arange(n) / 9.0 + rs.uniform(0, 6)) + walk * 0.2 + 0.02 * rs.standard_normal(n)), 80.0,
                   400.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ragged_rows():
    """one contour per entry of COUNTS, a few exact zeros in the rows of ZERO_ROWS"""
    rows = []
    for i, n in enumerate(COUNTS):
        v = contour(n, 100 + i)
        if n in ZERO_ROWS:
            v[np.random.RandomState(n).choice(n, size=1 if n < 10 else 3, replace=False)] = 0.0
        v.setflags(write=False)
        rows.append(v)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def ragged_references():
    """(decompose_ref, decompose_f64) of every row of ragged_rows(), computed once"""
    return tuple((decompose_ref(v), decompose_f64(v)) for v in ragged_rows())


def ulp32(x):
    """the spacing of float32 at |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))
