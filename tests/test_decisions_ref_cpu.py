"""The yardstick of tests/test_gpu_decisions.py checked on the CPU: the references of tests/_decisions.py against
oracle_cpu and torch.bucketize, and the input builders against the conditions the GPU cases rely on."""
import math

import numpy as np
import pytest
import torch

import _decisions as D
from oracle import oracle_cpu


def _bin_sets(nbins):
    n = nbins - 1
    lin = torch.linspace(-3, 3, n)
    log = torch.from_numpy(np.exp(np.linspace(np.log(40.0), np.log(800.0), n)).astype(np.float32)).log()
    dup = torch.linspace(-2, 2, n).clone()
    dup[1::3] = dup[0::3][: len(dup[1::3])]           # runs of two equal edges
    return {"lin": lin, "log": log, "dup": torch.sort(dup).values}


def test_ref_durations_matches_the_oracle_off_the_risky_cells():
    g = torch.Generator().manual_seed(5)
    B, L = 8, 3000
    p = torch.rand(B, L, generator=g) * 2.4 - 0.3
    p[1] = p[1] * 0.1 - 0.2                           # rounds to zeros: guard
    mask = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        mask[b, L - 311 * b:] = b > 0
    r = D.ref_durations(p, mask)
    want, guarded = oracle_cpu.round_durations(p.clone(), mask)
    assert torch.equal(r["dur"][~r["risky"]], want.long()[~r["risky"]])
    assert sorted(guarded) == torch.nonzero(r["guard"]).flatten().tolist() and 1 in guarded
    assert torch.equal(r["cum"], torch.cumsum(r["dur"], 1)) and torch.equal(r["totals"], r["dur"].sum(1))
    # uniform p in [-0.3, 2.1]: about 2e-5 of the cells expected within the risky band, far below the 0.1 % the GPU cases allow
    share = float(r["risky"].float().mean())
    print("risky share", share)
    assert share <= 1e-3


def test_ref_durations_guard_threshold_and_forced():
    # sum == n_valid // 2 fires, one above does not; odd and even n_valid; n_valid 1 and 0
    rows, masks, fires = [], [], []
    L = 12
    for n_valid in (0, 1, 6, 7):
        for extra in (0, 1):
            k = torch.zeros(L)
            s = n_valid // 2 + extra
            if n_valid:
                k[0] = s
            m = torch.arange(L) >= n_valid
            rows.append(torch.log1p(k)); masks.append(m); fires.append(s <= n_valid // 2 if n_valid else True)
    p, mask = torch.stack(rows), torch.stack(masks)
    r = D.ref_durations(p, mask)
    assert not r["risky"].any()
    assert r["guard"].tolist() == [int(f) for f in fires]
    want, guarded = oracle_cpu.round_durations(p.clone(), mask)
    assert torch.equal(r["dur"], want.long()) and sorted(guarded) == torch.nonzero(r["guard"]).flatten().tolist()
    forced = torch.tensor([[3, 0, -2, 5], [0, 0, 0, 0]])
    f = D.ref_durations(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.bool), forced)
    assert f["dur"].tolist() == [[3, 0, 0, 5], [0, 0, 0, 0]] and f["cum"].tolist() == [[3, 3, 3, 8], [0, 0, 0, 0]]
    assert f["guard"].tolist() == [0, 0] and f["totals"].tolist() == [8, 0]


def test_halfway_rows_are_never_risky():
    k = torch.arange(21, dtype=torch.float64)
    for sign in (-1.0, 1.0):
        v = k + 0.5 + sign * 2.0 ** -10 * (k + 1.5)
        p = torch.log1p(v).float()[None]
        r = D.ref_durations(p, torch.zeros(1, 21, dtype=torch.bool))
        assert not r["risky"].any()
        assert torch.equal(r["dur"][0], (k + (1 if sign > 0 else 0)).long())


@pytest.mark.parametrize("cap", [None, 50, 1])
def test_ref_regulate_matches_the_oracle(cap):
    g = torch.Generator().manual_seed(22)
    B, L, H = 4, 23, 8
    x = torch.randn(B, L, H, generator=g)
    dur = torch.randint(0, 7, (B, L), generator=g)
    dur[3, 10:] = 0
    want, wmask = oracle_cpu.length_regulator(x, dur.int(), cap if cap else 1e9)
    y, mask = D.ref_regulate(x, dur, want.shape[1])
    assert torch.equal(y, want) and torch.equal(mask, wmask)
    top = int(dur.sum(1).max())
    y2, mask2 = D.ref_regulate(x, dur, top + 9)             # T past every total: zero rows, mask set
    assert torch.equal(y2[:, :want.shape[1]], want) and not y2[:, top:].any() and mask2[:, top:].all()


def test_ref_bucket_embed_is_bucketize_and_an_ordered_fp32_sum():
    g = torch.Generator().manual_seed(3)
    B, T, H, nb = 2, 40, 8, 66
    bins = torch.linspace(-3, 3, nb - 1)
    x, emb = torch.randn(B, T, H, generator=g), torch.randn(nb, H, generator=g)
    pe, spk = torch.randn(T, H, generator=g), torch.randn(B, H, generator=g)
    src = torch.randn(B, T, generator=g)
    src[0, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0])
    y, idx = D.ref_bucket_embed(x, src, bins, emb, 1.3, -0.2, pe, spk, torch.float32)
    assert torch.equal(idx, torch.bucketize(src * 1.3 + (-0.2), bins))
    assert idx[0, :3].tolist() == [nb - 1, nb - 1, 0]        # torch sends NaN to the LAST bucket
    assert torch.equal(y, ((x + emb[idx]) + pe[None]) + spk[:, None])
    y16, _ = D.ref_bucket_embed(x, src, bins, emb, 1.3, -0.2, pe, spk, torch.bfloat16)
    xr = x.to(torch.bfloat16).float()
    assert torch.equal(y16, (((xr + emb[idx]) + pe[None]) + spk[:, None]).to(torch.bfloat16).float())
    yu, iu = D.ref_bucket_embed(x, src[:, 0], bins, emb, 1.0, 0.0, None, None, torch.float32, per_utt=True)
    assert (iu == iu[:, :1]).all() and iu[0, 0] == nb - 1
    ya, ia = D.ref_bucket_embed(x, None, None, None, 1.0, 0.0, pe, None, torch.float32)
    assert ia is None and torch.equal(ya, x + pe[None])


def test_nan_goes_to_the_last_bucket_in_torch():
    bins = torch.linspace(-1, 1, 7)
    assert int(torch.bucketize(torch.tensor(float("nan")), bins)) == 7
    assert int(torch.bucketize(torch.tensor(float("inf")), bins)) == 7
    assert int(torch.bucketize(torch.tensor(float("-inf")), bins)) == 0
    assert int(torch.bucketize(torch.tensor(-0.0), torch.tensor([0.0]))) == 0   # on the edge: -0.0 == 0.0


@pytest.mark.parametrize("nbins", [2, 3, 65, 66, 256, 513, 514, 1000])
@pytest.mark.parametrize("std,mean", [(1.0, 0.0), (1.3, -0.2)])
def test_edge_inputs_land_on_and_next_to_every_edge(nbins, std, mean):
    for name, raw in _bin_sets(nbins).items():
        bins = D.snap_bins(raw, std, mean)
        assert bool((bins[1:] >= bins[:-1]).all())
        d = D.edge_inputs(bins, std, mean)
        v_on, v_lo, v_hi = (D.bucket_value(d[k], std, mean) for k in ("on", "below", "above"))
        assert torch.equal(v_on, bins), name                        # after snapping, a src sits exactly on every edge
        assert bool((v_lo < bins).all()) and bool((v_hi > bins).all())
        # the sum's operands set the grid v lives on: one ulp of the larger of |e| and |e - mean| (cancellation near e = 0)
        ulp = torch.from_numpy(np.spacing(np.maximum(np.abs(bins.numpy()), np.abs(bins.numpy() - np.float32(mean))).astype(np.float32)))
        ulp = torch.maximum(ulp, torch.tensor(2.0 ** -149))
        assert bool(((bins - v_lo) <= 8 * ulp).all()) and bool(((v_hi - bins) <= 8 * ulp).all()), name
        if std == 1.0 and mean == 0.0:
            assert torch.equal(v_lo, torch.nextafter(bins, torch.tensor(-math.inf)))
            assert torch.equal(v_hi, torch.nextafter(bins, torch.tensor(math.inf)))
        k = torch.arange(nbins - 1)
        # on an edge and just below it: the edges strictly below v; just above: also every edge equal to it
        assert torch.equal(torch.bucketize(v_on, bins), torch.searchsorted(bins, bins))
        assert torch.equal(torch.bucketize(v_lo, bins), torch.searchsorted(bins, bins))
        assert torch.equal(torch.bucketize(v_hi, bins), torch.searchsorted(bins, bins, right=True))
        if name != "dup":
            assert torch.equal(torch.bucketize(v_on, bins), k) and torch.equal(torch.bucketize(v_hi, bins), k + 1)
        ex = torch.bucketize(D.bucket_value(d["extra"], std, mean), bins)
        assert ex[:3].tolist() == [nbins - 1, 0, nbins - 1] and ex[-2:].tolist() == [0, nbins - 1]
        assert torch.isnan(d["extra"][2]) and math.copysign(1.0, float(d["extra"][3])) < 0


def test_fma_discriminating_inputs_exist_and_discriminate():
    bins = torch.linspace(-3, 3, 255)
    std, mean = 1.3, -0.2
    src, per_edge = D.fma_discriminating_inputs(bins, std, mean)
    print("FMA-discriminating src:", len(src), "at", per_edge, "of 255 edges")
    assert len(src) >= 32
    two = torch.bucketize(D.bucket_value(src, std, mean), bins)
    one = (src.double() * float(np.float32(std)) + float(np.float32(mean))).float()
    assert bool((two != torch.bucketize(one, bins)).all())
