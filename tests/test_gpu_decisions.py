"""The forward's decision kernels (`-m gpu`), each against a plain reference of the same operation (tests/_decisions.py, itself
checked on the CPU by tests/test_decisions_ref_cpu.py), exactly, at every branch of the kernel and at the edges of its shapes:
duration rounding / guard / prefix sums, the length regulator, bucketise + embedding add (stand-alone launch, the per-utterance and
teacher-target entry points, and the copy inside the predictor launch), phone embedding and the speaker projection.

Outputs are pre-filled with a sentinel (NaN / 0x5a bytes) and carry one guard row behind the end: a row the kernel never writes
and a write past the end both fail.  Comparisons are on raw bits unless a derived bound is stated.

Outside the contract, not tested: non-finite or int32-overflowing duration predictions (the reference's own `.int()` is
platform-defined there)."""

import numpy as np
import pytest
import torch

import _decisions as D
import _gpu as G
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.config import Fs2Config, preset
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
from oracle import oracle_cpu
from test_gpu_forward import MEL_TOL_FP32

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(G.F32, id="fp32"), pytest.param(G.BF16, id="bf16")]


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# =====================================================================================================================
# durations
# =====================================================================================================================
DUR_L = [1, 63, 255, 256, 257, 1024, 1025, 3000]


def _ragged(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(0, L + 1, (B,), generator=g)
    n[0] = L
    return torch.arange(L)[None, :] >= n[:, None]


def _check_durations(p, mask, forced=None, constructed=True):
    r = D.ref_durations(p, mask, forced)
    st, dur, cum, tot, grd, intact = G.durations_s(p, mask, forced)
    assert st == 0 and intact
    risky = r["risky"]
    share = float(risky.float().mean())
    print(f"durations B={p.shape[0]} L={p.shape[1]}: risky cells {int(risky.sum())} ({share:.2e})")
    if constructed:
        assert not risky.any()
    assert share <= 1e-3
    assert torch.equal(dur.long()[~risky], r["dur"][~risky])
    clean = ~risky.any(1)
    assert int((~clean).sum()) <= 1
    assert torch.equal(cum.long()[clean], r["cum"][clean])
    assert torch.equal(tot.long()[clean], r["totals"][clean])
    assert torch.equal(grd.long()[clean], r["guard"][clean])


@pytest.mark.parametrize("L", DUR_L)
def test_durations_guard_threshold(L):
    """Per utterance sum == n_valid // 2 (the guard fires) and one above (it does not), for the largest even and odd n_valid that fit,
    n_valid = 1 and n_valid = 0; p = log1p(k), within 1e-6 of the integer.  The ones sit spread over the valid phones, the last one
    included (every scan trip contributes); masked cells carry a duration of 2, which neither the sum nor the count may see.
    One more row is all masked with p = 0 in every cell (what the engine feeds): totals 0, guard as the reference."""
    even, odd = L - L % 2, L - (1 - L % 2)
    rows, masks = [], []
    for n_valid in (0, 1, even, odd):
        for extra in (0, 1):
            k = torch.zeros(L)
            s = min(n_valid // 2 + extra, n_valid)
            if s:
                k[torch.linspace(0, n_valid - 1, s).round().long()] = 1
            assert int(k.sum()) == s
            m = torch.arange(L) >= n_valid
            k[m] = 2
            rows.append(torch.log1p(k))
            masks.append(m)
    rows.append(torch.zeros(L))                       # all masked with p = 0 everywhere, as the engine's masked_fill leaves it: totals 0
    masks.append(torch.ones(L, dtype=torch.bool))
    _check_durations(torch.stack(rows), torch.stack(masks))


@pytest.mark.parametrize("L", DUR_L)
def test_durations_halfway(L):
    """v = k + 0.5 -+ 2**-10 (k + 1.5) for k = 0..20: both sides of every half, far outside what an ulp of expf moves."""
    k = torch.arange(21, dtype=torch.float64)
    pat = torch.cat([k + 0.5 - 2.0 ** -10 * (k + 1.5), k + 0.5 + 2.0 ** -10 * (k + 1.5)])
    B = 4
    p = torch.stack([torch.log1p(pat[(torch.arange(L) + 11 * b) % 42]).float() for b in range(B)])
    _check_durations(p, _ragged(B, L, seed=L))


@pytest.mark.parametrize("L", DUR_L)
def test_durations_random(L):
    B = 8
    g = torch.Generator().manual_seed(100 + L)
    p = torch.rand(B, L, generator=g) * 2.4 - 0.3
    p[1] = p[1] * 0.1 - 0.2      # rounds to zeros: the guard fires
    _check_durations(p, _ragged(B, L, seed=200 + L), constructed=False)


@pytest.mark.parametrize("L", DUR_L)
def test_durations_forced(L):
    """Forced durations with zeros and negatives: dur = max(forced, 0) (the kernel clamps), prefix sums of the clamped values, no guard."""
    B = 5
    g = torch.Generator().manual_seed(300 + L)
    forced = torch.randint(-3, 9, (B, L), generator=g)
    forced[1] = 0
    forced[2] = -1
    _check_durations(rnd(B, L, seed=L), _ragged(B, L, seed=400 + L), forced=forced)


# =====================================================================================================================
# length regulator
# =====================================================================================================================
def _check_regulate(dtype, x, dur, T):
    B, L, H = x.shape
    dur = torch.as_tensor(dur).long()
    ref, rmask = D.ref_regulate(D.rounded(x, G.tdt(dtype)), dur, T)
    st, y, mk = G.regulate_s(dtype, x.reshape(B * L, H), torch.cumsum(dur, 1), dur.sum(1), B, L, T, H)
    assert st == 0
    assert G.guard_intact(y) and G.guard_intact(mk), "write behind the end"
    assert torch.equal(mk[:B].cpu(), rmask.to(torch.uint8)), (L, T, H)
    assert torch.equal(G.bits(y[:B * T]), G.to_bits(ref.reshape(B * T, H), dtype)), (L, T, H)


def _durs(B, L, seed, hi=5):
    g = torch.Generator().manual_seed(seed)
    dur = torch.randint(0, hi, (B, L), generator=g)
    tail = min(L, 64)
    dur[0, L - tail:] = torch.randint(0, 3, (tail,), generator=g)   # zeros and short phones among the LAST 64
    dur[0, L - 1] = 2
    if B > 1:
        dur[1, L // 2:] = 0                                          # trailing run of zeros
        dur[1, L - 1] = 1 if L > 64 else 0                           # ... closed by the very last phone on the long shapes
    return dur


def _t_values(dur):
    top = int(dur.sum(1).max())
    return sorted({1, 2, 63, 64, 65, 77, top, top + 7, max(1, top - 5), max(1, top // 2) | 1})


REG_H = [(G.BF16, h) for h in (8, 64, 256, 264, 512, 768, 1024)] + [(G.F32, h) for h in (4, 64, 128, 132, 256, 768, 1024)]


@pytest.mark.parametrize("dtype,H", REG_H, ids=[f"{'bf16' if d == G.BF16 else 'fp32'}-H{h}" for d, h in REG_H])
def test_regulate_copy_paths(dtype, H):
    """Two rows per wave (a row of at most 512 bytes) and one row per wave, at the last width of the first and the first of the
    second; T = 1, 2, odd, 63 / 64 / 65 (a workgroup is 4 waves x 16 rows), past every total and below the largest."""
    B, L = 3, 65
    x = rnd(B, L, H, seed=H)
    dur = _durs(B, L, seed=H + 1)
    for T in _t_values(dur):
        _check_regulate(dtype, x, dur, T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [1, 64, 65, 128, 1024, 1025, 2000])
def test_regulate_phone_counts(dtype, L):
    """One to sixteen ballot registers (L <= 1024) and the binary search (L > 1024), the interesting durations among the last 64 phones."""
    B = 3
    for H in (64, 512):
        x = rnd(B, L, H, seed=L + H)
        dur = _durs(B, L, seed=L, hi=3)
        top = int(dur.sum(1).max())
        for T in sorted({max(1, top), top + 3, max(1, top - 5), 65}):
            _check_regulate(dtype, x, dur, T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern", ["leading_zeros", "trailing_zeros", "zero_runs", "total_zero", "one_phone_1500", "all_ones", "random"])
def test_regulate_duration_patterns(dtype, pattern):
    for L in (40, 1000, 1100):
        B, H = 3, 64 if L == 40 else 8
        g = torch.Generator().manual_seed(L)
        dur = torch.randint(1, 4, (B, L), generator=g)
        if pattern == "leading_zeros":
            dur[:, : L // 3] = 0
            dur[1, : L - 1] = 0
        elif pattern == "trailing_zeros":
            dur[:, L - L // 3:] = 0
            dur[1, 1:] = 0
        elif pattern == "zero_runs":
            for s in range(0, L, 7):
                dur[:, s:s + 4] = 0
            dur[2, 5:L - 5] = 0
        elif pattern == "total_zero":
            dur[1] = 0
        elif pattern == "one_phone_1500":
            dur[:] = 0
            dur[0, L - 1] = 1500
            dur[1, 0] = 1500
            dur[2, L // 2] = 1500
        elif pattern == "all_ones":
            dur[:] = 1
        else:
            dur = torch.randint(0, 7, (B, L), generator=g)
            dur[2, 10:] = 0
        x = rnd(B, L, H, seed=L + 3)
        top = int(dur.sum(1).max())
        for T in (top, top + 9, max(1, top - 11)):
            _check_regulate(dtype, x, dur, T)


@pytest.mark.parametrize("dtype,H", [(G.BF16, 4), (G.F32, 6)], ids=["bf16-H4", "fp32-H6"])
def test_regulate_declines_rows_that_are_not_16_byte_multiples(dtype, H):
    B, L, T = 2, 5, 9
    dur = torch.ones(B, L, dtype=torch.long)
    st, y, mk = G.regulate_s(dtype, rnd(B * L, H), torch.cumsum(dur, 1), dur.sum(1), B, L, T, H)
    assert st == _lib.FS2_ERR_SHAPE
    assert G.untouched(y) and G.untouched(mk)


# =====================================================================================================================
# bucketise + embedding add
# =====================================================================================================================
STD, MEAN = 1.3, -0.2
NBINS = [2, 3, 65, 66, 256, 513, 514, 1000]


def bin_set(kind, nbins):
    n = nbins - 1
    if kind == "lin":
        return torch.linspace(-3, 3, n)
    if kind == "log":   # log-spaced, as the CWT pitch head's bins
        return torch.from_numpy(np.exp(np.linspace(np.log(40.0), np.log(800.0), n)).astype(np.float32)).log()
    dup = torch.linspace(-2, 2, n).clone()
    dup[1::3] = dup[0::3][: len(dup[1::3])]
    return torch.sort(dup).values


def _check_bucket(entry, dtype, src, bins, emb, std, mean, pe, spk, x, B, T):
    """x (B, T, H); src (B, T) or (B,) for the per-utterance entry, or None: the add-only form."""
    H = x.shape[-1]
    ref, ridx = D.ref_bucket_embed(x, src, bins, emb, std, mean, pe, spk, G.tdt(dtype), per_utt=entry == "utt")
    st, y, idx = G.bucket_embed_s(entry, dtype, x.reshape(B * T, H), None if src is None else src.reshape(-1), bins, emb, std, mean,
                                  pe, spk, B, T, H)
    assert st == 0
    assert G.guard_intact(y) and G.guard_intact(idx), "write behind the end"
    if src is not None:
        got = idx[:B * T, 0].cpu().long()
        bad = torch.nonzero(got != ridx.reshape(-1)).flatten()
        assert len(bad) == 0, (entry, len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), ridx.reshape(-1)[bad[:5]].tolist())
    assert torch.equal(G.bits(y[:B * T]), G.to_bits(ref.reshape(B * T, H), dtype)), (entry, H, B, T)


def _fill(src, n, seed):
    """src padded with random values to n entries."""
    return torch.cat([src, rnd(n - len(src), seed=seed, scale=1.5)]) if n > len(src) else src


@pytest.mark.parametrize("kind", ["lin", "log", "dup"])
@pytest.mark.parametrize("nbins", NBINS)
def test_bucket_values_on_and_next_to_every_edge(nbins, kind):
    """1 .. 999 edges: every ballot-register count, the last size of the register path (512 edges), the first of the binary
    search.  For every edge a value exactly on it, the nearest reachable below and above; +-inf, -0.0, 0.0, far below and above.
    Row and teacher-target entries with std = 1.3, mean = -0.2; the per-utterance entry (std 1, mean 0: the value as it is).
    The edges are SNAPPED (D.snap_bins: moved a few ulp onto values fl(fl(src * std) + mean) can take), since with std != 1 most
    edges of a linspace are not reachable exactly; the neighbours are the nearest reachable values, nextafter at std 1, mean 0.
    Unsnapped linspace edges with std != 1 are the business of test_bucket_value_is_multiply_then_add_not_fma."""
    H = 64
    emb = rnd(nbins, H, seed=nbins)
    for entry, std, mean in (("row", STD, MEAN), ("target", STD, MEAN), ("utt", 1.0, 0.0)):
        bins = D.snap_bins(bin_set(kind, nbins), std, mean)
        src = D.edge_rows(bins, std, mean)
        assert len(src) == 3 * (nbins - 1) + 7           # a value ON every edge exists
        src = src[~torch.isnan(src)]                     # NaN: test_bucket_nan_goes_to_the_last_bucket
        for dtype in (G.F32, G.BF16):
            if entry == "utt":
                B, T = len(src), 3
                _check_bucket(entry, dtype, src, bins, emb, std, mean, None, None, rnd(B, T, H, seed=7), B, T)
            else:
                B = 3
                T = (len(src) + B - 1) // B
                s = _fill(src, B * T, seed=5).reshape(B, T)
                _check_bucket(entry, dtype, s, bins, emb, std, mean, rnd(T, H, seed=8), rnd(B, H, seed=9), rnd(B, T, H, seed=7), B, T)


@pytest.mark.parametrize("entry", ["row", "target", "utt"])
@pytest.mark.parametrize("nbins", NBINS)
def test_bucket_nan_goes_to_the_last_bucket(nbins, entry):
    """torch.bucketize tests !(edge >= v): NaN lands in bucket nbins - 1."""
    H, B, T = 64, 4, 9
    std, mean = (1.0, 0.0) if entry == "utt" else (STD, MEAN)
    bins = bin_set("lin", nbins)
    emb = rnd(nbins, H, seed=nbins)
    src = rnd(B, seed=1) if entry == "utt" else rnd(B, T, seed=1)
    src.reshape(-1)[::3] = float("nan")
    pe, spk = (None, None) if entry == "utt" else (rnd(T, H, seed=8), rnd(B, H, seed=9))
    ridx = torch.bucketize(D.bucket_value(src, std, mean), bins)
    assert int((ridx == nbins - 1).sum()) >= src.numel() // 3
    for dtype in (G.F32, G.BF16):
        _check_bucket(entry, dtype, src, bins, emb, std, mean, pe, spk, rnd(B, T, H, seed=7), B, T)


@pytest.mark.parametrize("M", [1, 31, 32, 33, 300])
@pytest.mark.parametrize("H", [4, 64, 252, 256, 260, 768, 1024, 1028, 1536])
def test_bucket_row_widths_and_row_counts(H, M):
    """One to four unrolled 256-column chunks, the rolled loop (H > 1024), a partial last chunk; row counts around a workgroup's
    32 rows; with and without pe / spk; the add-only form."""
    nbins = 256
    B, T = {1: (1, 1), 31: (1, 31), 32: (2, 16), 33: (3, 11), 300: (3, 100)}[M]
    bins = D.snap_bins(bin_set("lin", nbins), STD, MEAN)
    emb = rnd(nbins, H, seed=H)
    src = _fill(D.edge_rows(bins, STD, MEAN)[: M // 2], M, seed=M)
    src = torch.where(torch.isnan(src), torch.zeros(()), src).reshape(B, T)
    x, pe, spk = rnd(B, T, H, seed=1), rnd(T, H, seed=2), rnd(B, H, seed=3)
    for dtype in (G.F32, G.BF16):
        for use_pe, use_spk in ((True, True), (False, False), (True, False), (False, True)):
            _check_bucket("row", dtype, src, bins, emb, STD, MEAN, pe if use_pe else None, spk if use_spk else None, x, B, T)
        _check_bucket("target", dtype, src, bins, emb, STD, MEAN, pe, spk, x, B, T)
        _check_bucket("row", dtype, None, None, None, 1.0, 0.0, pe, spk, x, B, T)      # pred = None: add only
        _check_bucket("row", dtype, None, None, None, 1.0, 0.0, None, spk, x, B, T)
        _check_bucket("utt", dtype, src[:, 0].contiguous(), D.snap_bins(bin_set("lin", nbins), 1.0, 0.0), emb, 1.0, 0.0, None, None, x, B, T)


@pytest.mark.parametrize("entry", ["row", "target"])
def test_bucket_value_is_multiply_then_add_not_fma(entry):
    """Inputs on which fl(fl(src * std) + mean) and the single-rounding src * std + mean fall on different sides of an edge."""
    nbins, H = 256, 64
    bins = torch.linspace(-3, 3, nbins - 1)
    src, per_edge = D.fma_discriminating_inputs(bins, STD, MEAN)
    print(f"{len(src)} FMA-discriminating inputs at {per_edge} of {nbins - 1} edges")
    assert len(src) >= 32, "vacuous: no input tells the two roundings apart"
    B, T = 2, len(src)
    s = torch.stack([src, src.flip(0)])
    for dtype in (G.F32, G.BF16):
        _check_bucket(entry, dtype, s, bins, rnd(nbins, H, seed=2), STD, MEAN, rnd(T, H, seed=3), rnd(B, H, seed=4), rnd(B, T, H, seed=5), B, T)


@pytest.mark.parametrize("entry", ["row", "target", "utt"])
@pytest.mark.parametrize("nbins", [256, 700])
def test_bucket_random_values(nbins, entry):
    H, B, T = 256, 5, 61
    std, mean = (1.0, 0.0) if entry == "utt" else (STD, MEAN)
    src = rnd(B, seed=3, scale=2.0) if entry == "utt" else rnd(B, T, seed=3, scale=2.0)
    pe, spk = (None, None) if entry == "utt" else (rnd(T, H, seed=8), rnd(B, H, seed=9))
    for dtype in (G.F32, G.BF16):
        _check_bucket(entry, dtype, src, bin_set("lin", nbins), rnd(nbins, H, seed=1), std, mean, pe, spk, rnd(B, T, H, seed=7), B, T)


# =====================================================================================================================
# the copy of the edge count inside the predictor launch (no op-level entry: through the model)
# =====================================================================================================================
def _model(cfg, sd, precision):
    from lightningfastspeech2_amd.model import FastSpeech2
    return FastSpeech2(cfg, sd, precision=precision, device="cuda:0")


def _cpu(d):
    return {k: ({kk: vv.cpu() for kk, vv in v.items()} if isinstance(v, dict) else v.cpu()) for k, v in d.items()}


def _batch(inp):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in inp.items() if k in ("phones", "speaker") or k.startswith("priors_")}


@pytest.mark.parametrize("level", ["frame", "phone"])
@pytest.mark.parametrize("prec", ["bf16", "fp32x3"])
@pytest.mark.parametrize("arch", ["c2", "ref-default"])
def test_tail_values_on_edges(arch, prec, level):
    """The first variance's `bins` are replaced by values its own predictions take (fl(fl(pred * std) + mean), the pad rows' common
    value among them), so that half a bin count of valid rows and every pad row sit exactly ON an edge.  The stand-alone launch
    (knob 1320, debug taps) must give torch.bucketize of the engine's own returned prediction, no exclusions; the predictor
    launch's tail (knob 1321) must give the stand-alone launch's bits in every output."""
    base = preset(arch).to_dict()
    if level == "phone":
        base["variance_levels"] = ["phone", "frame", "frame"]
    cfg = Fs2Config(**base)
    nb, var = cfg.variance_nbins, cfg.variances[0]
    std, mean = cfg.stats[var]["std"], cfg.stats[var]["mean"]
    sd = synth_state_dict(cfg, 6, randomize_norm=True, duration_bias=1.45)
    B, L, lengths = 4, 200, [200, 150, 199, 170]
    batch = _batch(synth_inputs(cfg, B, L, seed=91, lengths=lengths))
    key, mkey = f"variances_{var}", "src_mask" if level == "phone" else "tgt_mask"

    m = _model(cfg, sd, prec)
    m.engine.set_tuning(1320)
    out = _cpu(m(batch, inference=True))
    pad = out[mkey]
    vals = D.bucket_value(out[key], std, mean)
    assert int((~pad).sum()) >= 2 * nb and bool(pad.any())
    padv = D.bucket_value(torch.zeros(()), std, mean)
    assert bool((vals[pad] == padv).all())
    uniq = torch.unique(vals[~pad])
    uniq = uniq[uniq != padv]
    assert len(uniq) >= nb - 2
    pick = uniq[torch.linspace(0, len(uniq) - 1, nb - 2).round().long()]
    bins = torch.sort(torch.cat([pick, padv.reshape(1)])).values
    assert len(torch.unique(bins)) == nb - 1
    sd2 = dict(sd)
    sd2[f"variance_adaptor.encoders.{var}.bins"] = bins.numpy().copy()

    m2 = _model(cfg, sd2, prec)
    m2.engine.set_debug(True)
    m2.engine.set_tuning(1320)
    a = _cpu(m2(batch, inference=True))
    got = m2.engine.debug_tensor(f"bucket_{var}").cpu().long()
    v2 = D.bucket_value(a[key], std, mean)
    on_edge = torch.isin(v2, bins)
    print(f"{arch} {prec} {level}: {int(on_edge[~a[mkey]].sum())} valid rows on an edge, {int(a[mkey].sum())} pad rows")
    assert int(on_edge[~a[mkey]].sum()) >= nb // 2 and bool(on_edge[a[mkey]].all())
    assert torch.equal(got, torch.bucketize(v2, bins))
    m2.engine.set_debug(False)
    outs = {}
    try:
        for knob in (1320, 1321):
            m2.engine.set_tuning(knob)
            outs[knob] = _cpu(m2(batch, inference=True))
    finally:
        m2.engine.set_tuning(1321)
    for k, t in outs[1320].items():
        if torch.is_tensor(t):
            assert torch.equal(t, outs[1321][k]), k
    assert torch.isfinite(outs[1321]["mel"]).all()
    # the runs without the debug taps (whose other launches may differ from the debug run's) meet the condition too
    v3, pad3 = D.bucket_value(outs[1321][key], std, mean), outs[1321][mkey]
    assert int(torch.isin(v3, bins)[~pad3].sum()) >= nb // 2 and bool(torch.isin(v3, bins)[pad3].all())


@pytest.mark.parametrize("nbins", [513, 514, 700])
def test_tail_is_taken_up_to_512_edges_and_declined_beyond(nbins):
    """512 edges still fit the tail's eight edge registers per lane; from 513 edges on the predictor launch declines the tail and
    the stand-alone launch's binary search runs (shown by the count of stand-alone launches with knob 1320 against 1321).  Either
    way the buckets are torch.bucketize of the engine's own prediction, the two knobs agree bit for bit, and the fp32 engine under
    the oracle's durations agrees with the oracle's buckets (flips reported and handled as tests/test_gpu_forward.py
    test_fp32_matches_oracle does)."""
    cfg = Fs2Config(**{**preset("c2").to_dict(), "variance_nbins": nbins})
    sd = synth_state_dict(cfg, 3, randomize_norm=True, duration_bias=1.5)
    inp = synth_inputs(cfg, 3, 48, seed=53, lengths=[48, 30, 11])
    batch = _batch(inp)
    rowops = _lib.K_ROWOPS
    m = _model(cfg, sd, "bf16")
    n, outs = {}, {}
    try:
        for knob in (1321, 1320):
            m.engine.set_tuning(knob)
            m.engine.profile_enable(rowops, True)
            outs[knob] = _cpu(m(batch, inference=True))
            n[knob] = m.engine.profile_read(rowops)["launches"]
    finally:
        m.engine.profile_enable(rowops, False)
        m.engine.set_tuning(1321)
    assert n[1320] - n[1321] == (len(cfg.variances) if nbins - 1 <= 512 else 0), n
    for k, t in outs[1320].items():
        if torch.is_tensor(t):
            assert torch.equal(t, outs[1321][k]), k
    m.engine.set_debug(True)
    a = _cpu(m(batch, inference=True))
    for v in cfg.variances:
        want = torch.bucketize(D.bucket_value(a[f"variances_{v}"], cfg.stats[v]["std"], cfg.stats[v]["mean"]),
                               torch.as_tensor(sd[f"variance_adaptor.encoders.{v}.bins"]).float())
        assert torch.equal(m.engine.debug_tensor(f"bucket_{v}").cpu().long(), want), v

    ref = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"], return_intermediates=True)
    m32 = _model(cfg, sd, "fp32")
    m32.engine.set_debug(True)
    out = _cpu(m32.forward(batch, force_durations=ref["duration_rounded"]))
    assert torch.equal(out["tgt_mask"], ref["tgt_mask"])
    bflips = {v: int((m32.engine.debug_tensor(f"bucket_{v}").cpu().long() != ref["_intermediates"][f"bucket_{v}"]).sum()) for v in cfg.variances}
    for v in cfg.variances:
        want = torch.bucketize(D.bucket_value(out[f"variances_{v}"], cfg.stats[v]["std"], cfg.stats[v]["mean"]),
                               torch.as_tensor(sd[f"variance_adaptor.encoders.{v}.bins"]).float())
        assert torch.equal(m32.engine.debug_tensor(f"bucket_{v}").cpu().long(), want), v
    print(f"nbins {nbins}: stand-alone launches {n}, fp32 bucket flips against the oracle {bflips}")
    if sum(bflips.values()):   # the oracle sat within float noise of an edge: compare under ITS decisions
        out = _cpu(m32.forward(batch, force_durations=ref["duration_rounded"],
                               force_buckets={v: ref["_intermediates"][f"bucket_{v}"] for v in cfg.variances}))
    assert float((out["mel"] - ref["mel"]).abs().max()) <= MEL_TOL_FP32


def _same_bits(a, b):
    if a.is_floating_point():
        return torch.equal(G.bits(a), G.bits(b))
    return torch.equal(a, b)


def test_tail_sends_a_nan_prediction_to_the_last_bucket():
    """A NaN head bias makes every valid row's prediction NaN (pad rows stay the masked 0): the stand-alone launch puts them into
    bucket nbins - 1 as torch.bucketize does, and the tail inside the predictor launch gives the same bits in every output."""
    cfg = preset("c2")
    var, nb = cfg.variances[0], cfg.variance_nbins
    sd = dict(synth_state_dict(cfg, 3, randomize_norm=True, duration_bias=1.5))
    sd[f"variance_adaptor.encoders.{var}.predictor.linear.bias"] = np.full((1,), np.nan, dtype=np.float32)
    batch = _batch(synth_inputs(cfg, 3, 48, seed=53, lengths=[48, 30, 11]))
    m = _model(cfg, sd, "bf16")
    m.engine.set_debug(True)
    m.engine.set_tuning(1320)
    a = _cpu(m(batch, inference=True))
    pad = a["tgt_mask"]
    pred = a[f"variances_{var}"]
    assert bool(torch.isnan(pred[~pad]).all()) and bool((pred[pad] == 0).all()) and bool(pad.any())
    want = torch.bucketize(D.bucket_value(pred, cfg.stats[var]["std"], cfg.stats[var]["mean"]),
                           torch.as_tensor(sd[f"variance_adaptor.encoders.{var}.bins"]).float())
    assert bool((want[~pad] == nb - 1).all())
    assert torch.equal(m.engine.debug_tensor(f"bucket_{var}").cpu().long(), want)
    m.engine.set_debug(False)
    outs = {}
    try:
        for knob in (1320, 1321):
            m.engine.set_tuning(knob)
            outs[knob] = _cpu(m(batch, inference=True))
    finally:
        m.engine.set_tuning(1321)
    b = outs[1321]
    assert torch.isfinite(b["mel"]).all() and bool(torch.isnan(b[f"variances_{var}"][~b["tgt_mask"]]).all())
    for k, t in outs[1320].items():
        if torch.is_tensor(t):
            assert _same_bits(t, b[k]), k


# =====================================================================================================================
# phone embedding, speaker projection
# =====================================================================================================================
@pytest.mark.parametrize("L", [1, 19, 257])
@pytest.mark.parametrize("H", [4, 64, 260, 384, 768, 1024])
def test_embed_widths_lengths_and_ids(H, L):
    """Ids 0, n_phones - 1 and out of range (n_phones, -1, 2**40: row 0 is used, src_mask only where the id IS 0)."""
    B, V = 3, 40
    g = torch.Generator().manual_seed(H + L)
    phones = torch.randint(1, V, (B, L), generator=g)
    special = torch.tensor([0, V - 1, V, -1, 2 ** 40])
    flat = phones.reshape(-1)
    pos = torch.randperm(B * L, generator=g)[: min(B * L, 10)]
    flat[pos] = special[torch.arange(len(pos)) % 5]
    table, pe, spk = rnd(V, H, seed=30), rnd(L, H, seed=31), rnd(B, H, seed=32)
    row = torch.where((phones >= 0) & (phones < V), phones, torch.zeros((), dtype=torch.long))
    ref = (table[row] + pe[None]) + spk[:, None]
    for dtype in (G.F32, G.BF16):
        st, x, mk = G.embed_s(dtype, phones, table, pe, spk, V)
        assert st == 0 and G.guard_intact(x) and G.guard_intact(mk)
        assert torch.equal(mk[:B].cpu(), phones.eq(0).to(torch.uint8))
        assert torch.equal(G.bits(x[:B * L]), G.to_bits(ref.reshape(B * L, H), dtype))


@pytest.mark.parametrize("B,H", [(3, 7), (5, 67)])
@pytest.mark.parametrize("Din", [1, 63, 64, 65, 256, 512])
def test_speaker_projection_shapes(Din, B, H):
    """relu(W d + b) against float64.  Bound per output, from the formats: an fp32 sum of Din products plus the bias in any order
    is within 4 * 2**-24 * (Din + 2) * sum |w_k d_k| + 2**-24 |b| of the exact value; where the exact value lies below minus
    that bound the output is an exact zero."""
    assert (B * H) % 4
    dv, w, b = rnd(B, Din, seed=33 + Din), rnd(H, Din, seed=34, scale=Din ** -0.5), rnd(H, seed=35)
    st, out = G.spk_proj_s(dv, w, b)
    assert st == 0 and G.guard_intact(out)
    got = out[:B].cpu().double()
    s = dv.double() @ w.double().T + b.double()
    bound = 4 * 2.0 ** -24 * (Din + 2) * (dv.double().abs() @ w.double().abs().T) + 2.0 ** -24 * b.double().abs()
    err = (got - torch.relu(s)).abs()
    print(f"spk_proj Din={Din}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((got[s < -bound] == 0).all()) and bool((got >= 0).all())


# =====================================================================================================================
# CWT pitch head
# =====================================================================================================================
@pytest.mark.parametrize("ld", [10, 12])
@pytest.mark.parametrize("F", [64, 256, 384])
@pytest.mark.parametrize("T", [2, 255, 256, 257, 1536])
def test_cwt_head(T, F, ld):
    """mean_std = mean_std_linear(mean over ALL T rows of out_conv); s = sum of the 10 scales (pad rows 0, but counted in T);
    pred = (s - mean s) / (unbiased std s + 1e-7) * std_b + mean_b, against the same three lines in float64.

    Bounds from the formats (u = 2**-24; fp32 sums over T terms against the exact value, T u relative to the sum of magnitudes):
      mean_std: (T + F + 8) u (sum_c |w_c| mean_t |x_tc| + |b|)
      pred:     with S = max_t sum_j |spec_tj| and E = (T + 16) u S (covers the sum over the scales, the mean and the centring),
                the centred value is within E, the standard deviation within 3 E, z = d / (sd + 1e-7) within (1 + 3 |z|) E / sd, so
                |pred - ref| <= |std_b| (1 + 3 |z|) E / sd + (1 + |z|) bound(mean_std) + 4 u (|z std_b| + |mean_b|)
    The copied spectrogram (pad rows zeroed, columns past the 10th of a 12-wide row ignored) is exact."""
    B, u = 3, 2.0 ** -24
    lengths = [T, max(1, (2 * T) // 3), 1]
    mask = torch.arange(T)[None, :] >= torch.tensor(lengths)[:, None]
    spec = rnd(B * T, ld, seed=T + ld, scale=0.5)
    spec[:, 10:] = 1e3                                    # padding columns of the head GEMM's 12-wide rows: never summed
    ms_w, ms_b = rnd(2, F, seed=F, scale=F ** -0.5), torch.tensor([5.0, 0.3])
    oc = rnd(B, T, F, seed=T + F) + 0.25
    for dtype in (G.F32, G.BF16):
        x = D.rounded(oc, G.tdt(dtype)).double()
        st, ms, pred, so = G.cwt_head_s(dtype, oc.reshape(B * T, F), spec, mask, ms_w, ms_b, B, T, F)
        assert st == 0 and G.guard_intact(ms) and G.guard_intact(pred) and G.guard_intact(so)
        sp = spec[:, :10].reshape(B, T, 10).masked_fill(mask[..., None], 0)
        assert torch.equal(G.bits(so[:B * T]), G.bits(sp.reshape(B * T, 10)))
        ms_ref = x.mean(1) @ ms_w.double().T + ms_b.double()
        ms_bound = (T + F + 8) * u * (x.abs().mean(1) @ ms_w.double().abs().T + ms_b.double().abs())
        ms_err = (ms[:B].cpu().double() - ms_ref).abs()
        s = sp.double().sum(-1)
        d = s - s.mean(1, keepdim=True)
        sd = s.std(1, keepdim=True)
        z = d / (sd + 1e-7)
        ref = z * ms_ref[:, 1:2] + ms_ref[:, 0:1]
        E = (T + 16) * u * sp.double().abs().sum(-1).max(1, keepdim=True).values
        bound = (ms_ref[:, 1:2].abs() * (1 + 3 * z.abs()) * E / sd + (1 + z.abs()) * ms_bound.max(1, keepdim=True).values
                 + 4 * u * ((z * ms_ref[:, 1:2]).abs() + ms_ref[:, 0:1].abs()))
        err = (pred[:B].cpu().double() - ref).abs()
        print(f"cwt T={T} F={F} ld={ld} dtype={dtype}: mean_std err/bound {float((ms_err / ms_bound).max()):.3f}, pred err/bound {float((err / bound).max()):.3f}")
        assert bool((ms_err <= ms_bound).all())
        assert bool((err <= bound).all())


def test_cwt_head_declines_rows_narrower_than_the_ten_scales():
    B, T, F = 1, 4, 64
    st, ms, pred, so = G.cwt_head_s(G.F32, rnd(B * T, F), rnd(B * T, 8), None, rnd(2, F), rnd(2), B, T, F)
    assert st == _lib.FS2_ERR_SHAPE and G.untouched(ms) and G.untouched(pred) and G.untouched(so)
