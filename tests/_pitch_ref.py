"""CPU yardsticks of the F0 tracker (fs2_mel_pitch), written from the definition stated in include/fs2.h alone - YIN (de Cheveigne &
Kawahara 2002): the definition in float64, a sequential float32 restatement of its continuous stage (direct form, one running sum
per lag), the seeded test signals and the cases the CPU and the GPU test files share.  Nothing here is shared with the code under
test, and nothing is taken from pyworld: the tracker is not pinned against DIO + StoneMask.

A CASE is one batch of utterances at one geometry.  Its E_32 is the largest |d'_float32chain - d'_float64| over all of its frames
and lags: the error a plain float32 implementation of the same definition makes, the unit every bar of the GPU file is a multiple of.
"""
import functools
import math

import numpy as np

# (win_length, hop, sample rate) - n_fft = win_length
GEOMETRIES = {"small": (256, 64, 4000), "default": (1024, 256, 22050)}
F0_FLOOR, F0_CEIL, THRESHOLD = 71.0, 800.0, 0.1
# frames one workgroup owns (fs2_mel_pitch_tile_frames): the GPU file asserts that the library reports these, so that the lengths
# below sit at the kernel's seams and the CPU file checks the very cases the GPU file runs
TILE = {"small": 64, "default": 16}
# A window that is neither a multiple of the hop nor of 4 (n_fft 256): the kernel then sums a frame as one block of its own, with a
# short last step - another path of the code, so it gets a case; the exact-case and invariance tests stay on the two geometries above
ALL = dict(GEOMETRIES, ragged=(250, 64, 4000))
TILE["ragged"] = 64
MAX_FRAGILE = 0.02  # fragile frames are at most this share of a case's frames: a condition on the signals, not a measurement


def lags(sr, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    """(tau_min, tau_max)"""
    return max(2, int(math.floor(sr / f0_ceil))), int(math.ceil(sr / f0_floor))


def _gather(x, win, hop, tau_max, dtype):
    """the zero-extended signal and, per frame, the index of its first sample in it"""
    x = np.asarray(x, np.float32).astype(dtype)
    n = len(x)
    tf = 1 + n // hop
    left = win // 2
    xp = np.zeros(left + max(n, (tf - 1) * hop - left + win + tau_max + 2) + 1, dtype)
    xp[left:left + n] = x
    return xp, np.arange(tf) * hop  # frame t starts at t hop - win // 2, i.e. at t hop in xp


def difference64(x, win, hop, tau_max):
    """d (Tf, tau_max + 2) in float64"""
    xp, start = _gather(x, win, hop, tau_max, np.float64)
    idx = start[:, None] + np.arange(win)[None, :]
    a = xp[idx]
    return np.stack([((a - xp[idx + tau]) ** 2).sum(axis=1) for tau in range(tau_max + 2)], axis=1)


def difference32_chain(x, win, hop, tau_max):
    """d (Tf, tau_max + 2) as a sequential float32 program forms it: per lag one running sum over j = 0 .. W - 1, every operation
    rounded to float32"""
    xp, start = _gather(x, win, hop, tau_max, np.float32)
    taus = np.arange(tau_max + 2)
    acc = np.zeros((len(start), len(taus)), np.float32)
    for j in range(win):
        diff = xp[start + j][:, None] - xp[(start + j)[:, None] + taus[None, :]]
        acc += diff * diff
    return acc


def cmnd(d):
    """d' of d (Tf, NL), in d's own precision: the running sum sequential (np.cumsum), d'(0) = 1, 1 where the sum is 0"""
    d = np.asarray(d)
    tau = np.arange(1, d.shape[1]).astype(d.dtype)
    cum = np.cumsum(d[:, 1:], axis=1, dtype=d.dtype)
    out = np.ones_like(d)
    nz = cum != 0
    out[:, 1:][nz] = ((d[:, 1:] * tau[None, :])[nz] / cum[nz]).astype(d.dtype)
    return out


def pick(row, tau_min, tau_max, threshold):
    """step 4 on one frame's d' -> (tau or 0 when unvoiced, the walk's comparisons as a list of d'(tau + 1) - d'(tau))"""
    below = np.nonzero(row[tau_min:tau_max + 1] < threshold)[0]
    if len(below) == 0:
        return 0, []
    tau, steps = tau_min + int(below[0]), []
    while tau + 1 <= tau_max:
        steps.append(float(row[tau + 1]) - float(row[tau]))
        if not row[tau + 1] < row[tau]:
            break
        tau += 1
    return tau, steps


def refine(row, tau, sr):
    """step 5 -> (period tau + delta, f0, dmin, curv)"""
    a, b, c = float(row[tau - 1]), float(row[tau]), float(row[tau + 1])
    curv = a - 2.0 * b + c
    delta = min(0.5, max(-0.5, (a - c) / (2.0 * curv))) if curv > 0 else 0.0
    return tau + delta, sr / (tau + delta), b, curv


def track(cm, sr, tau_min, tau_max, threshold=THRESHOLD):
    """steps 4 and 5 on d' (Tf, NL) -> dict of per-frame arrays: tau (0 = unvoiced), period, f0, dmin, curv"""
    tf = len(cm)
    out = {k: np.zeros(tf) for k in ("period", "f0", "dmin", "curv")}
    out["tau"] = np.zeros(tf, np.int64)
    for t in range(tf):
        tau, _ = pick(cm[t], tau_min, tau_max, threshold)
        out["tau"][t] = tau
        if tau:
            out["period"][t], out["f0"][t], out["dmin"][t], out["curv"][t] = refine(cm[t], tau, sr)
        else:
            out["dmin"][t] = cm[t, tau_min:tau_max + 1].min()
    return out


def fragile(cm64, E, sr, tau_min, tau_max, threshold=THRESHOLD):
    """(Tf,) bool: frames whose decisions an error of E in d' may change - the float64 pick differs between the thresholds
    threshold - E and threshold + E; a comparison of the forward walk, the stopping one included, is closer than 2 E; or the
    frame is voiced and curv < 8 E"""
    out = np.zeros(len(cm64), bool)
    for t, row in enumerate(cm64):
        lo, hi = pick(row, tau_min, tau_max, threshold - E), pick(row, tau_min, tau_max, threshold + E)
        tau, steps = pick(row, tau_min, tau_max, threshold)
        bad = lo[0] != hi[0] or lo[0] != tau or any(abs(s) < 2 * E for s in steps + lo[1] + hi[1])
        if tau and not bad:
            bad = refine(row, tau, sr)[3] < 8 * E
        out[t] = bad
    return out


# ---- signals (all seeded)
def _harmonics(phase, f_inst, sr):
    """six harmonics at 1 / k amplitude of a fundamental with the given phase (radians per sample already integrated); a harmonic at
    or above sr / 2 cannot exist in a sampled signal and is left out (sample by sample on a glide)"""
    x = np.zeros_like(phase)
    for k in range(1, 7):
        x += np.where(k * f_inst < 0.5 * sr, np.sin(k * phase) / k, 0.0)
    return x


def _noisy(x, noise_db, seed):
    if noise_db is None:
        return x
    rs = np.random.RandomState(seed)
    return x + rs.standard_normal(len(x)) * np.sqrt(np.mean(x ** 2) * 10.0 ** (noise_db / 10.0))


def tone(n, f0, sr, seed, noise_db=-30.0, peak=0.6):
    """a harmonic tone at f0 Hz with seeded white noise noise_db below it (None: noiseless)"""
    rs = np.random.RandomState(seed)
    phase = 2.0 * np.pi * f0 * np.arange(n) / sr + rs.uniform(0, 2 * np.pi)
    x = _noisy(_harmonics(phase, np.full(n, float(f0)), sr), noise_db, seed + 1)
    return (x * (peak / np.abs(x).max())).astype(np.float32)


def glide(n, f_lo, f_hi, sr, seed, noise_db=-30.0, peak=0.6):
    """a linear glide of the fundamental from f_lo to f_hi"""
    f = np.linspace(f_lo, f_hi, n)
    x = _noisy(_harmonics(2.0 * np.pi * np.cumsum(f) / sr, f, sr), noise_db, seed)
    return (x * (peak / np.abs(x).max())).astype(np.float32)


def alternation(seg, f0, sr, seed):
    """voiced / white noise / exact zeros / voiced / exact zeros / white noise, `seg` samples each -> (x, kinds per segment)"""
    rs = np.random.RandomState(seed)
    kinds = ["voiced", "noise", "zero", "voiced", "zero", "noise"]
    parts = []
    for i, k in enumerate(kinds):
        if k == "voiced":
            parts.append(tone(seg, f0, sr, seed + 10 * i, noise_db=None))
        elif k == "noise":
            parts.append((0.2 * rs.standard_normal(seg)).astype(np.float32))
        else:
            parts.append(np.zeros(seg, np.float32))
    return np.concatenate(parts), kinds


# Fundamentals near the floor, in the middle and near the ceiling of each geometry's lag range: at 4 kHz 700 Hz is 5.7 samples a
# period and picks lag 6 (tau_min = 5), at 22050 Hz 760 Hz picks lag 29 (tau_min = 27).  The top tones are not arbitrary: steps 4 and
# 5 search integer lags and fit a parabola through three of them, and with a handful of samples a period that is biased by more than
# the 1 % tests/test_pitch_cpu.py holds the definition to for unlucky fractional periods (in float64: 760 Hz at 4 kHz is 2.6 % off);
# 700 Hz meets it (0.31 %).  The device bars do not depend on that: they compare with float64, whatever float64 picks.
TONES = {"small": (78.0, 250.0, 700.0), "default": (75.0, 240.0, 760.0), "ragged": (78.0, 250.0, 700.0)}


def seam_lengths(name):
    win, hop, sr = ALL[name]
    seam = TILE[name] * hop
    return [1, hop - 1, hop, hop + 1, win - 1, win, win + 1, seam - 1, seam, seam + 1, 2 * seam + 1]


def signals(name, case):
    """the rows of a case: "signals" - three tones, a glide, the alternation, an all-zero utterance; "lengths" - tones of every length
    at which the code takes another path"""
    win, hop, sr = ALL[name]
    seam = TILE[name] * hop
    lo, mid, hi = TONES[name]
    if case == "signals":
        n = 2 * seam + seam // 2 + 37
        return [tone(n, lo, sr, 1), tone(n - 101, mid, sr, 2), tone(n - 7, hi, sr, 3), glide(n, 1.1 * lo, 0.9 * hi, sr, 4),
                alternation(seam // 2 + 11, mid, sr, 5)[0], np.zeros(seam + 3 * hop + 1, np.float32)]
    if case == "lengths":
        return [tone(n, mid * (1.0 + 0.03 * i), sr, 20 + i) for i, n in enumerate(seam_lengths(name))]
    raise KeyError(case)


CASES = [(name, case) for name in GEOMETRIES for case in ("signals", "lengths")] + [("ragged", "signals")]


@functools.lru_cache(maxsize=None)
def reference(name, case):
    """The case's float64 yardstick, computed once and shared (treat as read-only): per row the float64 d' and its decisions, the
    case's E_32, per row the fragile frames at E = 2 E_32"""
    win, hop, sr = ALL[name]
    tau_min, tau_max = lags(sr)
    xs = signals(name, case)
    cm64 = [cmnd(difference64(x, win, hop, tau_max)) for x in xs]
    e32 = max(float(np.abs(cmnd(difference32_chain(x, win, hop, tau_max)).astype(np.float64) - c).max()) for x, c in zip(xs, cm64))
    E = 2.0 * e32
    rows = [dict(track(c, sr, tau_min, tau_max), cmnd=c, fragile=fragile(c, E, sr, tau_min, tau_max)) for c in cm64]
    return {"xs": xs, "rows": rows, "E_32": e32, "E": E, "tau_min": tau_min, "tau_max": tau_max,
            "frames": sum(len(c) for c in cm64), "n_fragile": int(sum(r["fragile"].sum() for r in rows))}
