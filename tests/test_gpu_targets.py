"""Training targets on the device (fs2_mel_snr, fs2_op_contour_finish, fs2_op_masked_row_mean, MelAnalyzer.snr / items) against
tests/_targets_ref.py and the reference's fixture tests/golden/frontend_targets.npz.

Bars.  SNR: the mapped error |delta out| * (g[i* + 1] - g[i*]) against the float64 yardstick is at most 2 * E_ref, E_ref being
the reference's own float32 path in that measure on the fixture (computed by _targets_ref.e_ref(), < 2e-6) and 2 the factor this
project gives its CPU models; against the fixture that bound plus E_ref.  A window whose float64 v3 lies within 1e-5 of a table
entry is left out (at most 2 % of a case's windows); NaN patterns are equal on all others.  Finishing, priors and the row mean:
1e-6 relative (of a contour: to the row's largest magnitude - a normalised contour crosses zero).  The SNR kernel owns 32 windows
per workgroup: lengths sit at that seam.

Seen on an MI355X (E_ref = 8.63e-7): 2.3e-7 ... 3.2e-7 against the yardstick, 5.6e-7 (1024 / 256) and 1.11e-6 (256 / 64) against the
reference's outputs; profiles/analysis_targets.md.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import _targets_ref as T
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.analysis import MelAnalyzer, finish_contour, masked_row_mean, segment_mean, slaney_mel_basis

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY, ICANARY, SLACK = 777.0, -7, 64
SNR_TILE = 32  # windows one workgroup of mel_snr_kernel owns (stated in its comment)
GEOMETRIES = {"default": (1024, 1024, 256), "small": (256, 256, 64)}


def table():
    return T.fixture()[0]["wada_table"]


class Snr:
    """fs2_mel_set_snr_table / fs2_mel_snr straight through the C ABI, every output buffer with canaries behind it"""

    def __init__(self, name, with_table=True):
        self.n_fft, self.win, self.hop = GEOMETRIES[name]
        self.lib, self.h = _lib.load(), C.c_void_p()
        basis = np.ones((8, self.n_fft // 2 + 1), np.float32)
        st = self.lib.fs2_mel_create(_lib.FS2_ABI_VERSION, self.n_fft, self.win, self.hop, 8, 1e-6, 0, basis.ctypes.data_as(C.c_void_p),
                                     C.byref(self.h))
        assert st == 0, self.lib.fs2_mel_last_error(self.h)
        if with_table:
            g = np.ascontiguousarray(table(), np.float64)
            assert self.lib.fs2_mel_set_snr_table(self.h, g.ctypes.data_as(C.c_void_p), len(g), -20) == 0

    def __del__(self):
        if self.h:
            self.lib.fs2_mel_destroy(self.h)
            self.h = None

    def run(self, wav, lengths, pn=True, Te_max=None, ws_short=0, null=(), B=None, frames=True):
        wav = np.ascontiguousarray(wav, np.float32)
        Bw, S = wav.shape
        B = Bw if B is None else B
        Te_max = -(-S // self.hop) if Te_max is None else Te_max
        w = torch.from_numpy(wav).to(DEV)
        ld = torch.tensor(lengths, dtype=torch.int32, device=DEV)
        out = torch.full((Bw * Te_max + SLACK,), CANARY, dtype=torch.float32, device=DEV)
        fr = torch.full((Bw + SLACK,), ICANARY, dtype=torch.int32, device=DEV)
        need = self.lib.fs2_mel_ws_bytes(self.h, Bw, S)
        ws = torch.zeros(need + SLACK, dtype=torch.uint8, device=DEV)
        args = {"wav": w, "snr": out}
        for k in null:
            args[k] = None
        st = self.lib.fs2_mel_snr(self.h, args["wav"], ld, B, S, int(pn), args["snr"], Te_max, fr if frames else None, ws, need - ws_short,
                                  torch.cuda.current_stream())
        torch.cuda.synchronize()
        out, fr = out.cpu().numpy(), fr.cpu().numpy()
        res = {"status": st, "snr": out[:-SLACK].reshape(Bw, Te_max), "frames": fr[:Bw],
               "canaries": bool((out[-SLACK:] == CANARY).all() and (fr[Bw:] == ICANARY).all() and (ws[need:].cpu().numpy() == 0).all())}
        res["untouched"] = bool(res["canaries"] and (out == CANARY).all() and (fr == ICANARY).all())
        return res


@functools.lru_cache(maxsize=None)
def snr_handle(name):
    return Snr(name)


def batch_of(xs, tail=37):
    """rows -> (B, S) with NaN in every sample at or past a row's length (S odd: rows start at every alignment)"""
    S = max(len(x) for x in xs) + tail
    S += 1 - S % 2
    wav = np.full((len(xs), S), np.nan, np.float32)
    for i, x in enumerate(xs):
        wav[i, :len(x)] = x
    return wav, [len(x) for x in xs]


def check_rows(name, xs, got, pn, bound, what):
    """every row of a device result against the float64 yardstick: mapped error, NaN pattern, zero rows past Te, the count; the
    near-ties left out are counted over the whole case"""
    n_fft, win, hop = GEOMETRIES[name]
    g, worst, ties, windows = table(), 0.0, 0, 0
    for b, x in enumerate(xs):
        want, v3, idx = T.wada_windows(x, win, hop, g, pn)
        te = len(want)
        assert got["frames"][b] == te == -(-len(x) // hop), (what, b)
        assert (got["snr"][b, te:] == 0).all(), (what, b)
        e, left_out = T.mapped_error(got["snr"][b, :te], want, v3, idx, g)
        worst, ties, windows = max(worst, e), ties + int(round(left_out * te)), windows + te
    print(f"{what} ({name}, peak_normalize {pn}): mapped error {worst:.2e}, bound {bound:.2e}, {ties} of {windows} windows left out")
    assert ties <= T.MAX_LEFT_OUT * windows, (what, ties, windows)
    assert worst <= bound, (what, worst, bound)
    return worst


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_snr_lengths_at_every_seam(name):
    n_fft, win, hop = GEOMETRIES[name]
    h = snr_handle(name)
    seam = SNR_TILE * hop
    lengths = [1, hop - 1, hop, hop + 1, win - 1, win, win + 1, seam - 1, seam, seam + 1, 2 * seam + 1]
    xs = [T.speech_like(n, 20.0, 300 + i, peak=0.7) for i, n in enumerate(lengths)]
    wav, lens = batch_of(xs)
    for pn in (False, True):
        o = h.run(wav, lens, pn)
        assert o["status"] == 0 and o["canaries"]
        check_rows(name, xs, o, pn, 2 * T.e_ref(), "lengths at the seams")
    assert list(o["frames"]) == [1, 1, 1, 2, 4, 4, 5, SNR_TILE, SNR_TILE, SNR_TILE + 1, 2 * SNR_TILE + 1]
    wide = h.run(wav, lens, True, Te_max=-(-wav.shape[1] // hop) + 3, frames=False)  # wider rows are zero-filled; snr_frames = NULL
    assert wide["status"] == 0 and wide["canaries"] and (wide["frames"] == ICANARY).all()
    for b in range(len(xs)):
        te = -(-lens[b] // hop)
        assert np.array_equal(wide["snr"][b, :te].view(np.uint32), o["snr"][b, :te].view(np.uint32)) and (wide["snr"][b, te:] == 0).all()


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_snr_fixture_signals(name):
    """the reference's own outputs: against the yardstick 2 E_ref, against the fixture 3 E_ref; the peak is 1, so peak_normalize
    changes nothing"""
    z, meta = T.fixture()
    c = meta["cases"][name]
    assert (c["n_fft"], c["win_length"], c["hop"]) == GEOMETRIES[name]
    h, g, E = snr_handle(name), table(), T.e_ref()
    xs = [z[f"{name}__{u}__wav"] for u in range(len(c["utterances"]))]
    wav, lens = batch_of(xs)
    on, off = h.run(wav, lens, True), h.run(wav, lens, False)
    assert on["status"] == off["status"] == 0 and on["canaries"] and off["canaries"]
    assert np.array_equal(on["snr"].view(np.uint32), off["snr"].view(np.uint32))
    check_rows(name, xs, on, True, 2 * E, "fixture signals against the yardstick")
    worst = 0.0
    for u, x in enumerate(xs):
        want, v3, idx = T.wada_windows(x, c["win_length"], c["hop"], g)
        e, left_out = T.mapped_error(on["snr"][u, :len(want)], z[f"{name}__{u}__wada"], v3, idx, g)
        assert left_out <= T.MAX_LEFT_OUT
        worst = max(worst, e)
    print(f"fixture signals against the reference's outputs ({name}): mapped error {worst:.2e}, bound {3 * E:.2e}")
    assert worst <= 3 * E


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_snr_special_signals(name):
    n_fft, win, hop = GEOMETRIES[name]
    h = snr_handle(name)
    rs = np.random.RandomState(5)
    gap = T.speech_like(12 * win + 77, 15.0, 11, peak=0.5)
    gap[3 * win + 5:5 * win + 9] = 0.0  # a run of more than win exact zeros: NaN windows inside
    const = np.full(5 * win + 3, 0.25, np.float32)  # v3 = 0: below the table, every window NaN
    noise = (0.3 * rs.standard_normal(20 * win + 1)).astype(np.float32)  # Gaussian: v3 at the table's non-monotone start
    tiny = (1e-30 * rs.standard_normal(2 * win)).astype(np.float32)  # squares underflow in fp32 without the peak scale
    xs = [gap, const, noise, tiny, np.zeros(3 * hop + 1, np.float32)]
    wav, lens = batch_of(xs)
    for pn in (True, False):
        o = h.run(wav, lens, pn)
        assert o["status"] == 0 and o["canaries"]
        check_rows(name, xs, o, pn, 2 * T.e_ref(), "special signals")
        te = [-(-n // hop) for n in lens]
        assert np.isnan(o["snr"][0, :te[0]]).sum() >= 4 and not np.isnan(o["snr"][0, :te[0]]).all()
        assert np.isnan(o["snr"][1, :te[1]]).all() and np.isnan(o["snr"][4, :te[4]]).all()
        assert np.isfinite(o["snr"][2, :te[2]]).any()
        if not pn:
            assert np.isnan(o["snr"][3, :te[3]]).all()


def test_snr_is_bitwise_batch_invariant():
    name = "default"
    n_fft, win, hop = GEOMETRIES[name]
    h = snr_handle(name)
    lens = [SNR_TILE * hop + 300, 777, 3 * SNR_TILE * hop - 1, hop, 5000]
    xs = [T.speech_like(n, 10.0 + 10 * i, 400 + i, peak=0.9) for i, n in enumerate(lens)]
    wav, lens = batch_of(xs)
    assert wav.shape[1] % 2 == 1 and np.isnan(wav[1, lens[1]:]).all()  # NaN past every length, rows at odd offsets
    for pn in (True, False):
        o = h.run(wav, lens, pn)
        assert o["status"] == 0 and o["canaries"]
        again = h.run(wav, lens, pn)
        assert np.array_equal(o["snr"].view(np.uint32), again["snr"].view(np.uint32))
        for b, x in enumerate(xs):
            te = -(-len(x) // hop)
            alone = h.run(x[None], [len(x)], pn)  # alone, S = its own length: aligned, the 16-byte loads
            assert alone["status"] == 0 and np.array_equal(alone["snr"][0].view(np.uint32), o["snr"][b, :te].view(np.uint32)), (pn, b)
            for pad in (1, 2, 3):  # another S: the row moves to every other alignment
                other = np.full((2, len(x) + pad), np.nan, np.float32)
                other[1, :len(x)] = x
                other[0, :5] = 1.0
                shifted = h.run(other, [5, len(x)], pn)
                assert np.array_equal(shifted["snr"][1, :te].view(np.uint32), o["snr"][b, :te].view(np.uint32)), (pn, b, pad)


def test_snr_argument_errors_write_nothing():
    h = snr_handle("default")
    x = T.speech_like(3000, 20.0, 1)[None]
    ARG, NOMEM, STATE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_NOMEM, _lib.FS2_ERR_STATE
    for kw, want in ((dict(ws_short=1), NOMEM), (dict(Te_max=11), ARG), (dict(null=("wav",)), ARG), (dict(null=("snr",)), ARG), (dict(B=0), ARG)):
        o = h.run(x, [3000], True, **kw)
        assert o["status"] == want and o["untouched"], (kw, o["status"])
        assert h.lib.fs2_mel_last_error(h.h) != b""
    bare = Snr("default", with_table=False)
    o = bare.run(x, [3000], True)
    assert o["status"] == STATE and o["untouched"] and b"fs2_mel_set_snr_table" in bare.lib.fs2_mel_last_error(bare.h)
    g = np.ascontiguousarray(table(), np.float64)
    for _ in range(2):  # the table may be set again
        assert bare.lib.fs2_mel_set_snr_table(bare.h, g.ctypes.data_as(C.c_void_p), len(g), -20) == 0
    ok = bare.run(x, [3000], True)
    assert ok["status"] == 0 and np.array_equal(ok["snr"].view(np.uint32), h.run(x, [3000], True)["snr"].view(np.uint32))


# ---- contour finishing
def finish_raw(values, frames, dur, silent, zim, amv, mean, std, with_prior=True):
    """fs2_op_contour_finish through the C ABI with canaries; frames / silent may be None (NULL)"""
    B, Tn = values.shape
    L = dur.shape[1]
    v = torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(DEV)
    d = torch.from_numpy(np.ascontiguousarray(dur, np.int32)).to(DEV)
    f = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=DEV)
    s = None if silent is None else torch.from_numpy(np.ascontiguousarray(silent, np.int32)).to(DEV)
    out = torch.full((B * Tn + SLACK,), CANARY, dtype=torch.float32, device=DEV)
    fo = torch.full((B + SLACK,), ICANARY, dtype=torch.int32, device=DEV)
    pr = torch.full((B + SLACK,), CANARY, dtype=torch.float32, device=DEV)
    st = _lib.load().fs2_op_contour_finish(v, f, d, s, B, Tn, L, int(zim), amv, mean, std, out, fo, pr if with_prior else None,
                                           torch.cuda.current_stream())
    torch.cuda.synchronize()
    out, fo, pr = out.cpu().numpy(), fo.cpu().numpy(), pr.cpu().numpy()
    assert st == 0 and (out[B * Tn:] == CANARY).all() and (fo[B:] == ICANARY).all() and (pr[B if with_prior else 0:] == CANARY).all()
    return out[:B * Tn].reshape(B, Tn), fo[:B], pr[:B]


def contour_rows(Tn, seed):
    """rows of (values, frames, durations, silent): every way a frame can be missing, at T = Tn"""
    rs = np.random.RandomState(seed)
    nan = np.nan

    def durs(total, L, zeros=0, negs=0):
        cuts = np.sort(rs.randint(0, total + 1, L - 1)) if L > 1 else np.array([], np.int64)
        d = np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64)
        for _ in range(zeros):
            d = np.insert(d, rs.randint(0, len(d) + 1), 0)
        for _ in range(negs):
            d = np.insert(d, rs.randint(0, len(d) + 1), -int(rs.randint(1, 9)))
        return d

    def vals():
        return (100.0 + 30.0 * rs.standard_normal(Tn)).astype(np.float32)
    rows = []
    L = lambda: int(rs.randint(1, min(Tn, 36) + 1))
    rows.append((vals(), Tn, durs(Tn, L()), None))                                    # nothing missing
    rows.append((np.full(Tn, nan, np.float32), Tn, durs(Tn, L()), None))              # all missing (NaN)
    v = vals(); v[:] = 0.0
    rows.append((v, Tn, durs(Tn, L(), zeros=2), None))                                # all zeros: missing only with zero_is_missing
    v = vals(); k = max(1, Tn // 5); v[:k] = nan; v[-k:] = nan; v[Tn // 2:Tn // 2 + k] = nan
    rows.append((v, Tn, durs(Tn, L()), None))                                         # runs at the start, the end and inside
    v = np.full(Tn, nan, np.float32); v[rs.randint(0, Tn)] = 42.0
    rows.append((v, Tn, durs(Tn, L()), None))                                         # a single present frame
    v = vals(); v[rs.rand(Tn) < 0.4] = 0.0; v[rs.rand(Tn) < 0.1] = nan
    d = durs(Tn, L(), zeros=2, negs=2)
    rows.append((v, Tn, d, (rs.rand(len(d)) < 0.4) | (d <= 0)))                       # silent phones, the empty ones among them
    d = durs(max(1, Tn - Tn // 3), L(), zeros=1)
    rows.append((v.copy(), Tn, d, rs.rand(len(d)) < 0.3))                             # sum d < frames
    d = durs(Tn + 7, L(), negs=1)
    rows.append((v.copy(), max(1, Tn - 2), d, rs.rand(len(d)) < 0.3))                 # sum d > frames, frames < T
    d = durs(Tn, L())
    rows.append((vals(), Tn, d, np.ones(len(d), bool)))                               # every phone silent
    rows.append((vals(), 0, durs(Tn, L()), None))                                     # no frames at all
    Lmax = max(len(r[2]) for r in rows)
    values = np.stack([r[0] for r in rows])
    dur = np.zeros((len(rows), Lmax), np.int64)
    sil = np.zeros((len(rows), Lmax), np.int64)
    for i, r in enumerate(rows):
        dur[i, :len(r[2])] = r[2]
        if r[3] is not None:
            sil[i, :len(r[3])] = r[3]
    return values, [r[1] for r in rows], dur, sil


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    scale = np.abs(want[ok]).max() if ok.any() else 0.0
    assert (np.abs(got[ok] - want[ok]) <= 1e-6 * scale).all(), (what, np.abs(got[ok] - want[ok]).max(), scale)


@pytest.mark.parametrize("Tn", [1, 63, 64, 65, 257, 1031])
def test_contour_finish(Tn):
    values, frames, dur, sil = contour_rows(Tn, Tn)
    assert dur.shape[1] <= 40
    for zim, amv, mean, std in ((False, 0.0, 0.0, 1.0), (True, 1e-7, 0.0, 1.0), (True, 0.0, 150.0, 40.0), (False, 1e-7, -3.0, 0.5)):
        for fr, sl in ((frames, sil), (None, sil), (frames, None)):
            out, fo, pr = finish_raw(values, fr, dur, sl, zim, amv, mean, std)
            for b in range(len(values)):
                want, F, prior = T.finish(values[b], dur[b], None if sl is None else sl[b], None if fr is None else fr[b], zim, amv, mean, std)
                what = (Tn, b, zim, amv, mean, std, fr is None, sl is None)
                assert fo[b] == F, what
                assert (out[b, F:] == 0).all(), what
                close(out[b, :F], want[:F], what)
                close(pr[b:b + 1], [prior], what)
            again = finish_raw(values, fr, dur, sl, zim, amv, mean, std)
            assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip((out, fo, pr), again))
            bare = finish_raw(values, fr, dur, sl, zim, amv, mean, std, with_prior=False)  # prior = NULL changes nothing else
            assert np.array_equal(bare[0].view(np.uint32), out.view(np.uint32)) and np.array_equal(bare[1], fo)


def test_contour_finish_at_its_limits():
    """T = 4096 frames and L = 2048 phones run; one more of either is FS2_ERR_SHAPE (tests/test_targets_cpu.py)"""
    rs = np.random.RandomState(9)
    values = (5.0 + rs.standard_normal((2, 4096))).astype(np.float32)
    values[:, rs.rand(4096) < 0.5] = np.nan
    values[1, :300] = np.nan
    values[1, -300:] = np.nan
    dur = np.full((2, 2048), 2, np.int64)
    sil = (rs.rand(2, 2048) < 0.2).astype(np.int64)
    out, fo, pr = finish_raw(values, [4096, 4000], dur, sil, False, 0.0, 5.0, 2.0)
    for b in range(2):
        want, F, prior = T.finish(values[b], dur[b], sil[b], [4096, 4000][b], False, 0.0, 5.0, 2.0)
        assert fo[b] == F and (out[b, F:] == 0).all()
        close(out[b, :F], want[:F], b)
        close(pr[b:b + 1], [prior], b)


def test_phone_level_against_the_reference():
    """finish at mean 0, std 1, then fs2_op_segment_mean with the stats, from the reference's own frame SNR: its phone outputs"""
    z, meta = T.fixture()
    st = meta["stats"]["snr"]
    for case, c in meta["cases"].items():
        for u in range(len(c["utterances"])):
            key = f"{case}__{u}"
            d, sil = z[key + "__duration"], z[key + "__silent"]
            raw = torch.from_numpy(z[key + "__wada"].astype(np.float32))[None].to(DEV)
            fin = finish_contour(raw, d[None], sil[None].astype(np.int32))
            assert int(fin["frames"][0]) == int(d.sum())
            close(fin["values"][0, :int(d.sum())].cpu().numpy(), z[f"{key}__frame__raw__snr"], key)
            for tag, (mean, std) in (("raw", (0.0, 1.0)), ("stats", (st["mean"], st["std"]))):
                got = segment_mean(fin["values"], torch.from_numpy(d[None]), fin["frames"], mean, std).cpu().numpy()[0]
                close(got, z[f"{key}__phone__{tag}__snr"], (key, tag))


def test_masked_row_mean():
    rs = np.random.RandomState(2)
    B, N = 6, 300  # more than one entry per thread
    values = (3.0 + rs.standard_normal((B, N))).astype(np.float32)
    skip = (rs.rand(B, N) < 0.3).astype(np.int32)
    skip[2] = 1       # everything skipped
    counts = [N, 0, N, 1000, 7, -3]  # 0 and negative: empty; 1000: clamped to N
    got = masked_row_mean(torch.from_numpy(values).to(DEV), counts, skip).cpu().numpy()
    for b in range(B):
        c = max(0, min(counts[b], N))
        keep = skip[b, :c] == 0
        want = values[b, :c][keep].astype(np.float64).mean() if keep.any() else np.nan
        close(got[b:b + 1], [want], b)
    assert np.isnan(got[[1, 2, 5]]).all() and np.isfinite(got[[0, 3, 4]]).all()
    plain = masked_row_mean(torch.from_numpy(values).to(DEV)).cpu().numpy()  # counts = skip = NULL
    close(plain, values.astype(np.float64).mean(axis=1), "plain")
    durs = torch.tensor([[3, 0, 5, 2], [1, 1, 0, 0]], dtype=torch.float32, device=DEV)  # the duration prior: durations as fp32
    pr = masked_row_mean(durs, [4, 2], torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0]])).cpu().numpy()
    assert pr[0] == np.float32(7.0 / 3.0) and pr[1] == 1.0


# ---- end to end
def test_items_collate_training_step():
    from lightningfastspeech2_amd.config import Fs2Config
    from lightningfastspeech2_amd.frontend import collate
    from lightningfastspeech2_amd.training import Trainer
    from lightningfastspeech2_amd.weights import synth_state_dict
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_small.npz"))
    cfg = Fs2Config.from_json(str(z["config_json"]))
    skw = json.loads(str(z["synth_json"]))
    g, hop, win = table(), cfg.hop_length, 1024
    an = MelAnalyzer(n_mels=cfg.n_mels, mel_basis=slaney_mel_basis(cfg.sampling_rate, 1024, cfg.n_mels, 0, 8000), hop_length=hop,
                     device=DEV, wada_table=g)
    with pytest.raises(RuntimeError, match="wada_values.npy"):
        MelAnalyzer(n_mels=cfg.n_mels, mel_basis=an.mel_basis, hop_length=hop, device=DEV).snr([np.ones(500, np.float32)])
    phones = [row[row != 0] for row in z["in_phones"]]
    durs = [z["in_duration"][i][:len(p)] for i, p in enumerate(phones)]
    rs = np.random.RandomState(8)
    audio = [T.speech_like(int(d.sum()) * hop + 100, 15.0 + 10 * i, 60 + i, peak=0.8) for i, d in enumerate(durs)]
    silent = [np.zeros(len(d), bool) for d in durs]
    pitch = []
    for i, d in enumerate(durs):
        silent[i][int(np.argmax(d > 0))] = True  # one silent phone that has frames
        te = -(-len(audio[i]) // hop)
        f0 = (120.0 + 30.0 * np.sin(np.arange(te) / 4.0) + rs.standard_normal(te)).astype(np.float32)
        f0[rs.rand(te) < 0.3] = 0.0  # unvoiced
        pitch.append(f0)
    names = list(cfg.variances)
    assert sorted(names) == ["energy", "pitch", "snr"]
    all_priors = names + ["duration"]
    items = an.items(audio, durs, silent=silent, pitch=pitch, stats=cfg.stats, variances=names, levels=("frame",) * 3, priors=all_priors)
    raw = an.snr(audio)
    energy = an(audio)["energy"].cpu().numpy().astype(np.float64)
    E = T.e_ref()
    for i, it in enumerate(items):
        total, d = int(durs[i].sum()), durs[i]
        assert sorted(it) == ["duration", "mel", "priors", "silence_mask", "unexpanded_silence_mask", "variances"]
        assert it["mel"].shape == (total, cfg.n_mels) and it["silence_mask"].shape == (total,) and it["silence_mask"].dtype == bool
        assert np.array_equal(it["unexpanded_silence_mask"], silent[i]) and np.array_equal(it["silence_mask"], T.expand(silent[i], d))
        # the device's raw SNR against the yardstick, then its finishing against the yardstick's rule
        want, v3, idx = T.wada_windows(audio[i], win, hop, g)
        dev_raw = raw["snr"][i, :len(want)].cpu().numpy()
        e, left_out = T.mapped_error(dev_raw, want, v3, idx, g)
        assert e <= 2 * E and left_out <= T.MAX_LEFT_OUT, (i, e, left_out)
        for name, src, kw in (("snr", dev_raw, dict(zero_is_missing=False, all_missing_value=0.0)),
                              ("pitch", pitch[i], dict(zero_is_missing=True, all_missing_value=1e-7))):
            fin, F, prior = T.finish(src, d, silent[i], None, mean=cfg.stats[name]["mean"], std=cfg.stats[name]["std"], **kw)
            assert F == total and it["variances"][name].shape == (total,) and it["variances"][name].dtype == np.float32
            close(it["variances"][name], fin[:F], (i, name))
            close([it["priors"][name]], [prior], (i, name, "prior"))
        close([it["priors"]["energy"]], [T.prior(energy[i, :total], it["silence_mask"])], (i, "energy prior"))
        close([it["priors"]["duration"]], [T.prior(d, silent[i])], (i, "duration prior"))
        it["phones"], it["speaker"] = phones[i], z["in_speaker"][i]
    batch = collate(items)
    Tm = int(max(d.sum() for d in durs))
    assert batch["mel"].shape == (3, Tm, cfg.n_mels)
    for name in names:
        assert batch[f"variances_{name}"].shape == (3, Tm) and bool(torch.isfinite(batch[f"variances_{name}"]).all())
        assert np.array_equal(batch[f"variances_{name}"][1, :len(items[1]["variances"][name])].numpy(), items[1]["variances"][name])
    for name in all_priors:
        assert len(batch[f"priors_{name}"]) == 3 and all(np.isfinite(float(v)) for v in batch[f"priors_{name}"])
    tr = Trainer(cfg, synth_state_dict(cfg, skw.pop("seed"), **skw), precision="fp32", **json.loads(str(z["hyper_json"])))
    losses = tr.training_step(batch)
    assert losses and all(np.isfinite(float(v)) for v in losses.values()), losses
    # phone level: (B, L) targets, the phone-level priors over the non-silent phones
    items = an.items(audio, durs, silent=silent, pitch=pitch, stats=cfg.stats, variances=names, levels=("phone",) * 3, priors=all_priors)
    for i, it in enumerate(items):
        d = durs[i]
        fin = T.finish(raw["snr"][i, :-(-len(audio[i]) // hop)].cpu().numpy(), d, silent[i])[0]
        pos = np.concatenate([[0], np.cumsum(np.maximum(d, 0))])
        pm = np.array([fin[pos[j]:pos[j + 1]].mean() if d[j] > 0 else 1e-7 for j in range(len(d))])
        close(it["variances"]["snr"], (pm - np.float32(cfg.stats["snr"]["mean"])) / np.float32(cfg.stats["snr"]["std"]), (i, "phone snr"))
        close([it["priors"]["snr"]], [T.prior(pm, silent[i])], (i, "phone snr prior"))
        it["phones"], it["speaker"] = phones[i], z["in_speaker"][i]
    batch = collate(items)
    L = max(len(d) for d in durs)
    for name in names:
        assert batch[f"variances_{name}"].shape == (3, L)
