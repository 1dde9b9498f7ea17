"""CPU yardsticks of the analysis front end (fs2_mel_*, lightningfastspeech2_amd/analysis.py), from the semantics of
include/fs2.h alone:

(a) ``mel_ref(..., dtype=torch.float64)``: torch.stft(center=True, pad_mode="constant") in float64 and the formulas;
(b) ``mel_ref(..., dtype=torch.float32)``: the CPU recipe the operator replaces - the same in float32;
(c) ``mel_chain``: the DFT and the mel product accumulated ONE TERM AT A TIME in float32 (product rounded, then the add rounded) -
    the least favourable legitimate order for an fp32 MFMA chain, and so the model the device is held to (2x, the factor
    tests/test_gpu_hifigan_fp16.py gives its CPU model).

All three return the LINEAR mel (T, n_mels), unclamped.  The figures are taken in the linear domain: per frame
max_m |mel - mel64| / max_m mel64, maximised over frames.  The log domain is unusable on narrow-band frames (on a 440 Hz tone
torch's own fp32 path is 2e-2 off float64 in log10 at entries six decades below the frame's peak while its linear figure is
1.2e-7), so |delta log10| is checked only at entries with mel64 >= 1e-3 * frame max and mel64 > clip.
"""
import numpy as np
import torch


class Geometry:
    def __init__(self, n_fft=1024, win_length=1024, hop=256, n_mels=80, clip=1e-6):
        self.n_fft, self.win_length, self.hop, self.n_mels, self.clip = n_fft, win_length, hop, n_mels, clip


def frame_counts(n, hop):
    """(mel frames, energy frames) of an utterance of n >= 1 samples"""
    return 1 + n // hop, -(-n // hop)


def scaled(x, peak_normalize, dtype):
    x = torch.as_tensor(np.asarray(x, np.float32)).to(dtype)
    peak = x.abs().max()
    return x * (1.0 / peak) if peak_normalize and peak > 0 else x


def stft_mag(x, g, dtype):
    """(T, n_fft / 2 + 1) magnitudes of the centred STFT: periodic Hann of win_length, zero padding at the utterance's own ends"""
    win = torch.hann_window(g.win_length, periodic=True, dtype=dtype)
    spec = torch.stft(x, g.n_fft, hop_length=g.hop, win_length=g.win_length, window=win, center=True, pad_mode="constant",
                      return_complex=True)
    return spec.abs().transpose(0, 1)


def mel_ref(x, g, basis, peak_normalize=True, dtype=torch.float64):
    """(a) / (b): the linear mel (T, n_mels) in `dtype`"""
    mag = stft_mag(scaled(x, peak_normalize, dtype), g, dtype)
    return (mag @ torch.as_tensor(np.asarray(basis)).to(dtype).transpose(0, 1)).numpy()


def dft_tables(g):
    """window[k] * cos / sin (2 pi f k / n_fft), (n_fft, n_fft / 2 + 1) each: float64, the phase reduced exactly"""
    win = np.zeros(g.n_fft)
    left = (g.n_fft - g.win_length) // 2
    n = np.arange(g.win_length)
    win[left:left + g.win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / g.win_length)
    r = (np.arange(g.n_fft)[:, None] * np.arange(g.n_fft // 2 + 1)[None, :]) % g.n_fft
    ang = 2.0 * np.pi * r / g.n_fft
    return win[:, None] * np.cos(ang), win[:, None] * np.sin(ang)


def frames_of(xs, g):
    """(T, n_fft): frame t = xs[t hop - n_fft / 2 + k], zero outside the utterance"""
    n = len(xs)
    T = 1 + n // g.hop
    pad = np.zeros(g.n_fft // 2 + (T - 1) * g.hop + g.n_fft, xs.dtype)
    pad[g.n_fft // 2:g.n_fft // 2 + n] = xs
    return np.stack([pad[t * g.hop:t * g.hop + g.n_fft] for t in range(T)])


def mel_chain(x, g, basis, peak_normalize=True):
    """(c): every sum a sequential float32 chain acc = fl(acc + fl(a * b)), tables rounded once from float64"""
    xs = scaled(x, peak_normalize, torch.float32).numpy()
    fr = frames_of(xs, g)
    cos64, sin64 = dft_tables(g)
    cos32, sin32 = cos64.astype(np.float32), sin64.astype(np.float32)
    re = np.zeros((fr.shape[0], cos32.shape[1]), np.float32)
    im = np.zeros_like(re)
    for k in range(g.n_fft):
        col = fr[:, k, None]
        re += col * cos32[k][None, :]
        im += col * sin32[k][None, :]
    mag = np.sqrt(re * re + im * im)
    b32 = np.asarray(basis, np.float32)
    mel = np.zeros((fr.shape[0], b32.shape[0]), np.float32)
    for f in range(b32.shape[1]):
        if b32[:, f].any():
            mel += mag[:, f, None] * b32[None, :, f]
    return mel


def linear_figure(mel, mel64):
    """max over frames of max_m |mel - mel64| / max_m mel64 (every entry takes part; a frame whose reference is all zero must be
    all zero)"""
    mel, mel64 = np.asarray(mel, np.float64), np.asarray(mel64, np.float64)
    assert mel.shape == mel64.shape, (mel.shape, mel64.shape)
    top = mel64.max(axis=1)
    err = np.abs(mel - mel64).max(axis=1)
    assert np.all(err[top == 0] == 0)
    return float((err[top > 0] / top[top > 0]).max()) if (top > 0).any() else 0.0


def log_selection(mel64, clip):
    """entries the log10 check keeps: within three decades of their frame's peak, and above the clamp"""
    mel64 = np.asarray(mel64, np.float64)
    return (mel64 >= 1e-3 * mel64.max(axis=1, keepdims=True)) & (mel64 > clip)


def log10_of(mel, clip):
    return np.log10(np.maximum(np.asarray(mel, np.float64), clip))


def log_figure(logmel, mel64, clip):
    """(max |logmel - log10(max(mel64, clip))| at the kept entries, share of entries kept)"""
    keep = log_selection(mel64, clip)
    d = np.abs(np.asarray(logmel, np.float64) - log10_of(mel64, clip))
    return (float(d[keep].max()) if keep.any() else 0.0), float(keep.mean())


def log10_f32(mel32, clip):
    """what a float32 path stores: log10 of the clamped float32 mel, rounded to float32"""
    return np.log10(np.maximum(np.asarray(mel32, np.float32), np.float32(clip))).astype(np.float32)


# ---- energy and the phone-level reduction
def energy_ref(x, g, peak_normalize=True):
    """float64: e[t] = sqrt(sum_{j = t hop}^{min(t hop + win, n) - 1} x~[j]^2 / win), ceil(n / hop) frames"""
    xs = scaled(x, peak_normalize, torch.float64).numpy()
    Te = -(-len(xs) // g.hop)
    return np.array([np.sqrt(np.sum(xs[t * g.hop:t * g.hop + g.win_length] ** 2) / g.win_length) for t in range(Te)])


def energy_chain(x, g, peak_normalize=True):
    """the same sum as a sequential float32 chain"""
    xs = scaled(x, peak_normalize, torch.float32).numpy()
    Te = -(-len(xs) // g.hop)
    out = np.zeros(Te, np.float32)
    for t in range(Te):
        acc = np.float32(0)
        for v in xs[t * g.hop:t * g.hop + g.win_length]:
            acc = np.float32(acc + np.float32(v * v))
        out[t] = np.sqrt(np.float32(acc / np.float32(g.win_length)))
    return out


def segment_mean_ref(values, frames, durations, mean=0.0, std=1.0, empty_value=1e-7, dtype=np.float64):
    """out[j] = (mean(values[pos_j : pos_j + d_j]) - mean) / std over the segment clipped to `frames`; empty -> empty_value.
    dtype float32: the sequential float32 chain of the same sums."""
    values = np.asarray(values, dtype)
    out = np.zeros(len(durations), dtype)
    pos = 0
    for j, d in enumerate(durations):
        lo, hi = min(pos, frames), min(pos + max(int(d), 0), frames)
        if hi > lo:
            acc = dtype(0)
            for v in values[lo:hi]:
                acc = dtype(acc + v)
            m = dtype(acc / dtype(hi - lo))
        else:
            m = dtype(empty_value)
        out[j] = dtype(dtype(m - dtype(mean)) / dtype(std))
        pos += max(int(d), 0)
    return out


# ---- the test inputs (a few tens of thousands of samples each)
def signal(kind, n, seed=0, sr=22050):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / sr
    if kind == "noise":
        x = 0.3 * rng.standard_normal(n)
    elif kind == "ramp":
        x = rng.standard_normal(n) * np.logspace(-5, 0, n)
    elif kind == "tone440":
        x = 0.9 * np.sin(2 * np.pi * 440.0 * t)
    elif kind == "tone3k":
        x = np.sin(2 * np.pi * 3000.0 * t) + 1e-3 * rng.standard_normal(n)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)
