"""CPU yardsticks of the training-target operators (fs2_mel_snr, fs2_op_contour_finish, fs2_op_masked_row_mean), written from the
semantics stated in include/fs2.h alone: the windowed WADA estimate per window in float64, the finishing rule through np.interp,
the priors formula mean(val[~silent]).  Nothing here is shared with the code under test."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_targets.npz")
EPS = 1e-20
NEAR_TIE = 1e-5     # a window whose float64 v3 lies this close to a table entry is left out: the lookup is discontinuous there
MAX_LEFT_OUT = 0.02  # ... at most this share of a case's windows
E_REF_BOUND = 2e-6  # the reference's own float32 path against float64, in the mapped measure: the fixture's figure stays below it


def fixture():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta_json"]))


def scaled32(x, peak_normalize=True):
    """x~ as the device forms it: the fp32 product of x and the fp32 reciprocal of the peak (scale 1 on an all-zero utterance)"""
    x = np.asarray(x, np.float32)
    peak = np.abs(x).max() if len(x) else np.float32(0)
    return x * (np.float32(1.0) / peak) if peak_normalize and peak > 0 else x


def wada_lookup(v3, table):
    """(out, i*) of one statistic: i* = max{i : g[i] < v3}; NaN when there is none, when it is the last entry, or unless out < K - 1"""
    g = np.asarray(table, np.float64)
    below = np.nonzero(g < v3)[0]
    if len(below) == 0 or below.max() == len(g) - 1:
        return np.nan, -1
    i = int(below.max())
    out = i + (v3 - g[i]) / (g[i + 1] - g[i])
    return (float(np.float32(out)), i) if out < len(g) - 1 else (np.nan, -1)


def wada_windows(x, win, hop, table, peak_normalize=True):
    """One utterance -> (out (Te,) float64 holding fp32-rounded values or NaN, v3 (Te,) float64, i* (Te,), -1 on NaN windows)"""
    xs = scaled32(x, peak_normalize)
    n = len(xs)
    te = -(-n // hop)
    out, v3s, idx = np.full(te, np.nan), np.full(te, np.nan), np.full(te, -1, np.int64)
    for t in range(te):
        seg32 = xs[t * hop:min(t * hop + win, n)]
        seg = np.abs(seg32.astype(np.float64))
        if not (seg > 0).any() or not ((seg32 * seg32) > 0).any():  # all zeros, or sum of squares zero in fp32
            continue
        a = np.maximum(seg, EPS)
        v3s[t] = np.log(max(EPS, a.mean())) - np.log(a).mean()
        out[t], idx[t] = wada_lookup(v3s[t], table)
    return out, v3s, idx


def mapped_error(got, want, v3, idx, table):
    """max over the windows that count of |got - want| * (g[i* + 1] - g[i*]): the error carried back to the statistic v3.  Windows
    within NEAR_TIE of a table entry are left out; on all others the NaN patterns must be equal.  -> (figure, share left out)"""
    g = np.asarray(table, np.float64)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == v3.shape, (got.shape, want.shape, v3.shape)
    tie = np.array([np.isfinite(v) and np.abs(g - v).min() < NEAR_TIE for v in v3], bool)
    keep = ~tie
    assert np.array_equal(np.isnan(got[keep]), np.isnan(want[keep])), (np.nonzero(np.isnan(got) != np.isnan(want))[0], v3)
    live = keep & ~np.isnan(want)
    if not live.any():
        return 0.0, float(tie.mean()) if len(tie) else 0.0
    slope = g[idx[live] + 1] - g[idx[live]]
    return float((np.abs(got[live] - want[live]) * slope).max()), float(tie.mean())


def expand(flags, durations):
    """phone flags -> frame flags (negative durations count as 0)"""
    return np.repeat(np.asarray(flags, bool), np.maximum(np.asarray(durations, np.int64), 0))


def finish(values, durations, silent=None, frames=None, zero_is_missing=False, all_missing_value=0.0, mean=0.0, std=1.0):
    """One row -> (out (T,) float64, F, prior).  y = the value where present, np.interp elsewhere (the first / last present value
    outside), all_missing_value when nothing is present; prior = mean(y[~silent frames]); out = (y - mean) / std, zeros from F."""
    v = np.asarray(values, np.float64)
    T = len(v)
    d = np.maximum(np.asarray(durations, np.int64), 0)
    sil = np.zeros(len(d), bool) if silent is None else np.asarray(silent) != 0
    F = int(min(d.sum(), T if frames is None else max(0, min(int(frames), T))))
    fsil = expand(sil, d)[:F]
    y = v[:F].copy()
    missing = np.isnan(y) | fsil
    if zero_is_missing:
        missing |= y == 0
    if missing.all():
        y[:] = np.float32(all_missing_value)
    else:
        at = np.arange(F)
        y[missing] = np.interp(at[missing], at[~missing], y[~missing])
    prior = y[~fsil].mean() if (~fsil).any() else np.nan
    out = np.zeros(T)
    out[:F] = (y - np.float32(mean)) / np.float32(std)
    return out, F, prior


def prior(val, silent):
    val = np.asarray(val, np.float64)
    keep = ~(np.asarray(silent) != 0)
    return val[keep].mean() if keep.any() else np.nan



def speech_like(n, snr_db, seed, peak=1.0):
    """gamma-amplitude (shape 0.4, the WADA model) "speech" + white Gaussian noise at snr_db, scaled to the given peak"""
    rs = np.random.RandomState(seed)
    s = rs.gamma(0.4, 1.0, n) * rs.choice([-1.0, 1.0], n)
    x = s + rs.standard_normal(n) * np.sqrt(np.mean(s ** 2) / 10.0 ** (snr_db / 10.0))
    return (x * (peak / np.abs(x).max())).astype(np.float32)


_E_REF = []


def e_ref():
    """The fixture's figure: the reference's own float32 path against the float64 yardstick in the mapped measure, over every
    fixture utterance.  Computed once; the constant the GPU tests' bounds are multiples of."""
    if not _E_REF:
        z, meta = fixture()
        g, worst = z["wada_table"], 0.0
        for case, c in meta["cases"].items():
            for u in range(len(c["utterances"])):
                out, v3, idx = wada_windows(z[f"{case}__{u}__wav"], c["win_length"], c["hop"], g)
                e, left_out = mapped_error(z[f"{case}__{u}__wada"], out, v3, idx, g)
                assert left_out <= MAX_LEFT_OUT, (case, u, left_out)
                worst = max(worst, e)
        _E_REF.append(worst)
    return _E_REF[0]
