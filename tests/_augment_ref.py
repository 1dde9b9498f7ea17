"""The three augmentation definitions of include/fs2.h ("Waveform augmentation") restated on the CPU, each twice:

- in float64 (the tables and responses as the device gets them: rounded once to float32, then exact), the reference;
- as a *sequential float32 chain*: the same sum accumulated in index order, one float32 multiply and one float32 add per term - the
  project's yardstick for what float32 arithmetic costs on this sum (the rule of test_gpu_analysis.py: a kernel may be off the
  float64 value by at most twice what the chain is).

Nothing here imports a signal-processing library; numpy only."""
import numpy as np

from lightningfastspeech2_amd.augment import resample_params, resample_table, resampled_length


def _frames(x, orig, width, K, n_frames, dtype):
    """F[i][q] = x[i * orig + q - width], zero outside [0, n)"""
    xp = np.zeros(width + max(n_frames - 1, 0) * orig + K + len(x), dtype=dtype)
    xp[width:width + len(x)] = x
    idx = np.arange(n_frames)[:, None] * orig + np.arange(K)[None, :]
    return xp[idx]


def resample_f64(x, orig_freq, new_freq, tab32=None):
    """y[i * new + p] = sum_q tab[p][q] x[i * orig + q - width], m = ceil(new * n / orig) outputs; float64 sums over the float32 table"""
    orig, new, width, K = resample_params(orig_freq, new_freq)
    tab = (resample_table(orig_freq, new_freq).astype(np.float32) if tab32 is None else tab32).astype(np.float64)
    m = resampled_length(len(x), orig, new)
    n_frames = -(-m // new)
    F = _frames(np.asarray(x, np.float64), orig, width, K, n_frames, np.float64)
    return (F @ tab.T).reshape(-1)[:m]


def resample_chain32(x, orig_freq, new_freq):
    orig, new, width, K = resample_params(orig_freq, new_freq)
    tab = resample_table(orig_freq, new_freq).astype(np.float32)
    m = resampled_length(len(x), orig, new)
    n_frames = -(-m // new)
    F = _frames(np.asarray(x, np.float32), orig, width, K, n_frames, np.float32)
    acc = np.zeros((n_frames, new), np.float32)
    for q in range(K):
        acc += F[:, q:q + 1] * tab[None, :, q]  # the product rounded, then the sum rounded
    return acc.reshape(-1)[:m]


def convolve_f64(x, h, mode="same"):
    """y[t] = sum_{k < R} h[k] x[t - k]; "same": t < n, "full": t < n + R - 1 (an empty utterance stays empty)"""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    if len(x) == 0:
        return np.zeros(0)
    y = np.convolve(x, h)
    return y[:len(x)] if mode == "same" else y


def convolve_chain32(x, h, mode="same"):
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    n, R = len(x), len(h)
    if n == 0:
        return np.zeros(0, np.float32)
    acc = np.zeros(n + R - 1, np.float32)
    for k in range(R):  # index order of the definition: k = 0 first
        acc[k:k + n] += h[k] * x
    return acc[:n] if mode == "same" else acc


def noise_scale_f64(x, snr_db):
    """rms / 10^(snr / 20) in float64 (0 for an empty utterance or snr = +inf)"""
    x = np.asarray(x, np.float64)
    if len(x) == 0 or np.isposinf(snr_db):
        return 0.0
    return float(np.sqrt(np.sum(x * x) / len(x)) / 10.0 ** (float(snr_db) / 20.0))


def add_noise_f32(x, z, scale32):
    """the float32 restatement given the scale: one multiply, one add"""
    return np.asarray(x, np.float32) + np.float32(scale32) * np.asarray(z, np.float32)


def pack(utts, lead=0, tail=0, fill=np.nan):
    """utterances back to back behind `lead` filler samples (odd offsets on purpose) -> (packed float32 with `tail` filler samples
    behind the last, offsets int64)"""
    off = np.cumsum([lead] + [len(u) for u in utts]).astype(np.int64)
    buf = np.full(int(off[-1]) + tail, fill, np.float32)
    for u, o in zip(utts, off):
        buf[o:o + len(u)] = u
    return buf, off
