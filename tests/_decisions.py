"""References and input builders for the forward's discrete decisions (durations, length regulator, bucketise + embedding).

Plain torch / numpy on the CPU, no GPU code: tests/test_gpu_decisions.py compares the HIP kernels with these, and
tests/test_decisions_ref_cpu.py checks these against oracle_cpu and torch.bucketize, so the yardstick is itself tested."""
import numpy as np
import torch

EPS32 = 2.0 ** -23


def rounded(x, dtype):
    """fp32 values of x after one round-to-nearest-even into `dtype` (torch.float32 / torch.bfloat16)."""
    x = torch.as_tensor(x).float()
    return x.to(torch.bfloat16).float() if dtype == torch.bfloat16 else x


# ---------------------------------------------------------------------------------------------------------------------
def ref_durations(p, mask, forced=None):
    """d = int(clamp(round_half_even(exp(p) - 1), 0)) in float64; guard: an utterance whose sum over valid phones is
    <= n_valid // 2 gets 1 at every valid phone (masked cells keep their own value); int64 prefix sums and totals.
    With `forced`: d = max(forced, 0), no guard.

    `risky` marks cells whose float64 value lies within 8 * 2**-23 * exp(p) of a half-integer: an fp32 expf (a few ulp of
    exp(p)) followed by one fp32 subtraction cannot move a value further than that, so outside these cells an fp32
    evaluation must round to the same integer.  (Derived from the formats, not measured.)

    Non-finite predictions and values beyond int32 are outside the contract: the reference's own `.int()` is
    platform-defined there."""
    p = torch.as_tensor(p).float()
    mask = torch.as_tensor(mask).bool()
    B, L = p.shape
    guard = torch.zeros(B, dtype=torch.int64)
    if forced is not None:
        dur = torch.as_tensor(forced).long().clamp(min=0)
        risky = torch.zeros(B, L, dtype=torch.bool)
    else:
        e = torch.exp(p.double())
        v = e - 1.0
        dur = torch.clamp(torch.round(v), min=0).long()
        risky = ((v - torch.floor(v)) - 0.5).abs() <= 8 * EPS32 * e
        for b in range(B):
            valid = ~mask[b]
            n_valid = int(valid.sum())
            if int(dur[b][valid].sum()) <= n_valid // 2:
                dur[b][valid] = 1
                guard[b] = 1
    cum = torch.cumsum(dur, 1)
    totals = dur.sum(1)
    return {"dur": dur, "cum": cum, "totals": totals, "guard": guard, "risky": risky}


def ref_regulate(x, dur, T):
    """x (B, L, H), dur (B, L) -> y (B, T, H): per utterance repeat_interleave, zero rows from total to T, truncated at T;
    mask (B, T) = t >= total with the UNtruncated total."""
    x = torch.as_tensor(x)
    dur = torch.as_tensor(dur).long()
    B, L, H = x.shape
    totals = dur.sum(1)
    y = x.new_zeros(B, T, H)
    for b in range(B):
        rep = torch.repeat_interleave(x[b], dur[b], dim=0)[:T]
        y[b, : rep.shape[0]] = rep
    mask = torch.arange(T)[None, :] >= totals[:, None]
    return y, mask


def bucket_value(src, std, mean):
    """v = src * std + mean as two separately rounded fp32 operations."""
    src = torch.as_tensor(src).float()
    return (src * torch.tensor(std, dtype=torch.float32)) + torch.tensor(mean, dtype=torch.float32)


def ref_bucket_embed(x, src, bins, emb, std, mean, pe, spk, dtype, per_utt=False):
    """x (B, T, H) fp32 (rounded into `dtype` first: what the kernel reads); src (B, T), or (B,) with per_utt, or None (add only).
    idx = torch.bucketize(src * std + mean, bins) (right=False);  y = ((x + emb[idx]) + pe[t]) + spk[b] in fp32, in that order,
    then one round-to-nearest-even into `dtype`.  Returns (y as fp32 values, idx (B, T) int64 or None)."""
    x = rounded(x, dtype)
    B, T, H = x.shape
    y, idx = x, None
    if src is not None:
        idx = torch.bucketize(bucket_value(src, std, mean), torch.as_tensor(bins).float())
        if per_utt:
            idx = idx.reshape(B, 1).expand(B, T)
        idx = idx.reshape(B, T)
        y = y + torch.as_tensor(emb).float()[idx]
    if pe is not None:
        y = y + torch.as_tensor(pe).float()[None, :T]
    if spk is not None:
        y = y + torch.as_tensor(spk).float()[:, None]
    return rounded(y, dtype), idx


# ---------------------------------------------------------------------------------------------------------------------
def _v32(src, std, mean):
    return (src.astype(np.float32) * np.float32(std)).astype(np.float32) + np.float32(mean)


def _ulp_window(center, k):
    """(n, 2k+1) fp32: center moved by -k..k units in the last place."""
    cols = [center]
    lo = hi = center
    for _ in range(k):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        cols = [lo] + cols + [hi]
    return np.stack(cols, 1).astype(np.float32)


def _key(f):
    """fp32 -> int64 in the numbers' own order (-0.0 and 0.0 share key 0)."""
    i = np.asarray(f, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def _from_key(k):
    k = np.asarray(k, dtype=np.int64)
    return np.where(k >= 0, k, (-k) | 0x80000000).astype(np.uint32).view(np.float32)


def _first_key(pred, n):
    """Per element, the smallest finite fp32 (as a key) for which the monotone predicate holds."""
    lo = np.full(n, int(_key(np.float32(-1e38))), dtype=np.int64)   # pred false
    hi = np.full(n, int(_key(np.float32(1e38))), dtype=np.int64)    # pred true
    assert not pred(_from_key(lo)).any() and pred(_from_key(hi)).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ok = pred(_from_key(mid))
        hi = np.where(ok, mid, hi)
        lo = np.where(ok, lo, mid)
    return hi


def snap_bins(bins, std, mean):
    """Edges moved (by a few ulp) onto values that fl(fl(src * std) + mean) can reach, so that a src exists exactly ON every edge."""
    b = np.asarray(bins, dtype=np.float32)
    src = ((b.astype(np.float64) - float(np.float32(mean))) / float(np.float32(std))).astype(np.float32)
    return torch.from_numpy(np.sort(_v32(src, std, mean)))


def edge_inputs(bins, std, mean):
    """fp32 src values around every edge e of `bins` under v = fl(fl(src * std) + mean):
      on[i]    v == e                       (NaN where no src reaches e exactly: see snap_bins)
      below[i] the largest reachable v < e  (nextafter(e, -inf) when std = 1, mean = 0)
      above[i] the smallest reachable v > e
    plus `extra`: +inf, -inf, NaN, -0.0, 0.0, one value below the first and one above the last edge.
    Returns a dict of fp32 tensors."""
    assert std > 0
    b = np.asarray(bins, dtype=np.float32)
    k_ge = _first_key(lambda s: _v32(s, std, mean) >= b, len(b))   # src -> v is monotone: bisect over the ordered fp32 numbers
    k_gt = _first_key(lambda s: _v32(s, std, mean) > b, len(b))
    at = _from_key(k_ge)
    on = np.where(_v32(at, std, mean) == b, at, np.float32(np.nan))
    below, above = _from_key(k_ge - 1), _from_key(k_gt)
    span = float(b[-1]) - float(b[0]) + 1.0
    far = np.array([(b[0] - span - mean) / std, (b[-1] + span - mean) / std], dtype=np.float32)
    extra = np.concatenate([np.array([np.inf, -np.inf, np.nan, -0.0, 0.0], dtype=np.float32), far])
    return {k: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for k, a in
            (("on", on), ("below", below), ("above", above), ("extra", extra))}


def edge_rows(bins, std, mean):
    """edge_inputs as one flat fp32 vector (NaN placeholders of unreachable `on` entries dropped)."""
    d = edge_inputs(bins, std, mean)
    on = d["on"][~torch.isnan(d["on"])]
    return torch.cat([on, d["below"], d["above"], d["extra"]])


def fma_discriminating_inputs(bins, std, mean):
    """src within +-40 ulp of (e - mean) / std for which the two-rounding fl(fl(src * std) + mean) and the one-rounding
    fl(src * std + mean) (the product of two fp32 numbers is exact in float64) fall into different buckets: a kernel that
    contracts the multiply-add into an FMA picks another embedding row on these."""
    b = np.asarray(bins, dtype=np.float32)
    s32, m32 = np.float32(std), np.float32(mean)
    c = ((b.astype(np.float64) - float(m32)) / float(s32)).astype(np.float32)
    win = _ulp_window(c, 40)
    two = _v32(win, std, mean)
    one = (win.astype(np.float64) * float(s32) + float(m32)).astype(np.float32)
    differ = np.searchsorted(b, two, side="left") != np.searchsorted(b, one, side="left")
    per_edge = int(differ.any(1).sum())
    src = np.unique(win[differ])
    return torch.from_numpy(src.astype(np.float32)), per_edge
