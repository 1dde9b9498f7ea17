"""The analysis front end on the device (fs2_mel_*, fs2_op_segment_mean, MelAnalyzer) against tests/_analysis_ref.py.

Bars, held by EVERY utterance on its own: the linear figure (per frame max_m |mel - mel64| / max_m mel64, maximised over the
utterance's frames, every entry taking part) is at most 2x the sequential-chain model's figure on that same utterance, the model
itself at most 1.5e-6; the |delta log10| at the kept entries (mel64 >= 1e-3 * frame max and mel64 > clip) is at most 2x the model's,
and on noise and ramp the selection keeps every entry.  Energy and the phone-level mean are held to 2x the float32 sequential-sum
model of the same sums against float64.

Maxima seen on an MI355X: in the docstrings of the tests below and in profiles/analysis_front_end.md.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import _analysis_ref as R
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.analysis import MelAnalyzer, segment_mean, slaney_mel_basis

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY, ICANARY, SLACK = 777.0, -7, 64
DEFAULT = R.Geometry()
SMALL = R.Geometry(n_fft=256, win_length=200, hop=64, n_mels=20)
# the kernel's other instantiations: a 32-frame tile with two mel tiles, a 16-frame tile (span close to the LDS limit) with four
GEOMETRIES = {"default": DEFAULT, "small": SMALL, "mid": R.Geometry(n_fft=2048, win_length=2048, hop=512, n_mels=40),
              "wide": R.Geometry(n_fft=2048, win_length=1024, hop=2048, n_mels=128)}


@functools.lru_cache(maxsize=None)
def basis_of(name):
    if name == "default":
        return slaney_mel_basis()
    if name == "mid":
        return slaney_mel_basis(22050, 2048, 40, 0, 8000)
    if name == "wide":
        return slaney_mel_basis(22050, 2048, 128, 0, None)
    return np.abs(np.random.RandomState(4).standard_normal((20, 129))).astype(np.float32) + 0.05  # dense: every bin is a DFT column


def geom(name):
    return GEOMETRIES[name]


class Mel:
    """fs2_mel_* straight through the C ABI, every output buffer with canaries behind it"""

    def __init__(self, name="default", kind=_lib.FS2_MEL_LOG10):
        self.g, self.basis, self.lib = geom(name), basis_of(name), _lib.load()
        self.h = C.c_void_p()
        g = self.g
        st = self.lib.fs2_mel_create(_lib.FS2_ABI_VERSION, g.n_fft, g.win_length, g.hop, g.n_mels, g.clip, kind,
                                     self.basis.ctypes.data_as(C.c_void_p), C.byref(self.h))
        assert st == 0, self.lib.fs2_mel_last_error(self.h)
        self.tile = self.lib.fs2_mel_tile_frames(self.h)

    def __del__(self):
        if self.h:
            self.lib.fs2_mel_destroy(self.h)
            self.h = None

    def run(self, wav, lengths, pn=False, energy=True, T_max=None, Te_max=None, ws_short=0, null=(), B=None):
        wav = np.ascontiguousarray(wav, np.float32)
        Bw, S = wav.shape
        B = Bw if B is None else B
        hop, nm = self.g.hop, self.g.n_mels
        T_max = 1 + S // hop if T_max is None else T_max
        Te_max = -(-S // hop) if Te_max is None else Te_max
        w = torch.from_numpy(wav).to(DEV)
        ld = torch.tensor(lengths, dtype=torch.int32, device=DEV)
        mel = torch.full((Bw * T_max * nm + SLACK,), CANARY, dtype=torch.float32, device=DEV)
        en = torch.full((Bw * Te_max + SLACK,), CANARY, dtype=torch.float32, device=DEV)
        mf = torch.full((Bw + SLACK,), ICANARY, dtype=torch.int32, device=DEV)
        ef = torch.full((Bw + SLACK,), ICANARY, dtype=torch.int32, device=DEV)
        need = self.lib.fs2_mel_ws_bytes(self.h, Bw, S)
        ws = torch.zeros(need + SLACK, dtype=torch.uint8, device=DEV)
        args = {"wav": w, "mel": mel, "mel_frames": mf, "energy": en if energy else None}
        for k in null:
            args[k] = None
        st = self.lib.fs2_mel_run(self.h, args["wav"], ld, B, S, int(pn), args["mel"], T_max, args["energy"], Te_max, args["mel_frames"],
                                  ef, ws, need - ws_short, torch.cuda.current_stream())
        torch.cuda.synchronize()
        mel, en, mf, ef = mel.cpu().numpy(), en.cpu().numpy(), mf.cpu().numpy(), ef.cpu().numpy()
        out = {"status": st, "mel": mel[:-SLACK].reshape(Bw, T_max, nm), "energy": en[:-SLACK].reshape(Bw, Te_max),
               "mel_frames": mf[:Bw], "energy_frames": ef[:Bw],
               "canaries": bool((mel[-SLACK:] == CANARY).all() and (en[-SLACK:] == CANARY).all() and (mf[Bw:] == ICANARY).all()
                                and (ef[Bw:] == ICANARY).all() and (ws[need:].cpu().numpy() == 0).all())}
        out["untouched"] = bool(out["canaries"] and (mel == CANARY).all() and (en == CANARY).all() and (mf == ICANARY).all()
                                and (ef == ICANARY).all())
        return out


@functools.lru_cache(maxsize=None)
def mel_handle(name, kind):
    return Mel(name, kind)


def batch_of(signals, tail=700):
    """rows of (kind, n, seed) -> (B, S) with NaN in every sample at or past a row's length"""
    xs = [R.signal(k, n, seed) for k, n, seed in signals]
    S = max(len(x) for x in xs) + tail
    wav = np.full((len(xs), S), np.nan, np.float32)
    for i, x in enumerate(xs):
        wav[i, :len(x)] = x
    return xs, wav, [len(x) for x in xs]


@functools.lru_cache(maxsize=None)
def refs(name, kind, n, seed, pn=False):
    """float64 reference and chain model of one utterance, computed once per session"""
    x = R.signal(kind, n, seed)
    return R.mel_ref(x, geom(name), basis_of(name), pn), R.mel_chain(x, geom(name), basis_of(name), pn)


def check_case(name, signals, pn=False, all_kept=True):
    """the bars of the module docstring on every utterance of one ragged batch; returns the maxima over the batch"""
    g = geom(name)
    xs, wav, lens = batch_of(signals)
    lin = mel_handle(name, _lib.FS2_MEL_LINEAR).run(wav, lens, pn)
    log = mel_handle(name, _lib.FS2_MEL_LOG10).run(wav, lens, pn)
    fig = {"lin_dev": 0.0, "lin_model": 0.0, "log_dev": 0.0, "log_model": 0.0, "kept": 1.0}
    for o in (lin, log):
        assert o["status"] == 0 and o["canaries"]
        assert not np.isnan(o["mel"]).any() and not np.isnan(o["energy"]).any()
    for i, (kind, n, seed) in enumerate(signals):
        T, Te = R.frame_counts(n, g.hop)
        for o in (lin, log):
            assert o["mel_frames"][i] == T and o["energy_frames"][i] == Te
            assert (o["mel"][i, T:] == 0).all() and (o["energy"][i, Te:] == 0).all()  # pad rows exactly zero
        m64, mc = refs(name, kind, n, seed, pn)
        ld, lm = R.linear_figure(lin["mel"][i, :T], m64), R.linear_figure(mc, m64)
        gd, keep = R.log_figure(log["mel"][i, :T], m64, g.clip)
        gm, _ = R.log_figure(R.log10_f32(mc, g.clip), m64, g.clip)
        print(f"{name} {kind} n={n}: linear device {ld:.2e} model {lm:.2e}; log10 device {gd:.2e} model {gm:.2e} at {keep:.3f}")
        if all_kept:
            assert keep == 1.0, (kind, n, keep)
        assert lm <= 1.5e-6 and ld <= 2 * lm, (kind, n, ld, lm)  # each utterance against its own model
        assert gd <= 2 * gm, (kind, n, gd, gm)
        # outside the kept entries the device's log is still the log of ITS linear mel (same launch arithmetic, logged in fp64)
        want = R.log10_of(lin["mel"][i, :T], g.clip)
        assert np.abs(log["mel"][i, :T] - want).max() <= 5e-7
        fig = {"lin_dev": max(fig["lin_dev"], ld), "lin_model": max(fig["lin_model"], lm), "log_dev": max(fig["log_dev"], gd),
               "log_model": max(fig["log_model"], gm), "kept": min(fig["kept"], keep)}
    print(f"{name}: case maxima {json.dumps({k: float('%.3g' % v) for k, v in fig.items()})}")
    return fig


def test_parity_default_geometry_at_the_tile_seams():
    """1024 / 1024 / 256 / 80: one length on each side of every seam of the 64-frame tiles, and one of 300 samples.
    Seen on an MI355X, device (model) per utterance: linear 9.6e-7 (8.0e-7), 8.7e-7 (8.5e-7), 1.17e-6 (1.05e-6), 2.3e-7 (2.2e-7); log10
    5.9e-7 (6.2e-7), 5.4e-7 (9.3e-7), 5.9e-7 (5.3e-7), 3.3e-7 (1.7e-7: the closest to its bar, 1.9x); every entry kept."""
    tile = mel_handle("default", _lib.FS2_MEL_LOG10).tile
    assert tile == 64
    check_case("default", (("noise", tile * 256 - 1, 1), ("ramp", tile * 256, 0), ("noise", (2 * tile + 2) * 256 + 17, 2), ("noise", 300, 3)))


def test_parity_small_geometry():
    """256 / 200 / 64 / 20 with a dense basis of its own (every bin a DFT column, a window shorter than n_fft).
    Seen on an MI355X: every utterance below its model - linear 0.9-2.1e-7 (models 2.3-5.7e-7), log10 0.7-1.9e-7 (1.8-4.4e-7); every
    entry kept."""
    assert mel_handle("small", _lib.FS2_MEL_LOG10).tile == 64
    check_case("small", tuple(("noise", n, n) for n in (1, 63, 64, 127, 5000)))


def test_parity_other_tiles():
    """2048 / 2048 / 512 / 40 runs 32-frame tiles with two mel tiles, 2048 / 1024 / 2048 / 128 16-frame tiles with four (the frame
    clamp of a half-filled MFMA row tile, a span of 128 KiB): one length on each side of the first seam of each.
    Seen on an MI355X: linear figure 5.8-6.6e-7 (models 6.6-7.5e-7) / 5.6-6.5e-7 (5.7-6.5e-7), log10 3.1-3.7e-7 (3.1-7.0e-7) /
    4.6-5.0e-7 (4.1-4.6e-7), every entry kept."""
    assert mel_handle("mid", _lib.FS2_MEL_LOG10).tile == 32 and mel_handle("wide", _lib.FS2_MEL_LOG10).tile == 16
    check_case("mid", (("noise", 32 * 512 - 1, 5), ("ramp", 32 * 512, 0)))
    check_case("wide", (("noise", 16 * 2048 - 1, 7), ("noise", 16 * 2048, 8)))


def test_parity_tones():
    """narrow-band frames: the linear bar on every entry, the log bar on the kept ones (8-14 % of them).
    Seen on an MI355X, 440 Hz / 3 kHz: linear 7.1e-7 (model 6.4e-7) / 7.6e-7 (8.4e-7), log10 at the kept entries 1.37e-5 (1.46e-5) /
    7.2e-6 (6.8e-6)."""
    fig = check_case("default", (("tone440", 24000, 0), ("tone3k", 24000, 0)), all_kept=False)
    assert 0.05 < fig["kept"] < 0.5


def test_silence():
    g = DEFAULT
    x = R.signal("noise", 8000, 7)
    x[6000:] = 0.0
    wav = np.full((2, 8700), np.nan, np.float32)
    wav[0, :5000] = 0.0
    wav[1, :8000] = x
    for pn in (False, True):
        o = mel_handle("default", _lib.FS2_MEL_LOG10).run(wav, [5000, 8000], pn)
        assert o["status"] == 0 and o["canaries"] and not np.isnan(o["mel"]).any() and not np.isnan(o["energy"]).any()
        assert o["mel_frames"].tolist() == [20, 32] and o["energy_frames"].tolist() == [20, 32]
        assert np.abs(o["mel"][0, :20] - np.log10(g.clip)).max() <= 1e-6 and (o["energy"][0] == 0).all()
        # frames whose whole window lies in the trailing zeros: t * 256 - 512 >= 6000; energy windows start at t * 256 >= 6000
        assert np.abs(o["mel"][1, 26:32] - np.log10(g.clip)).max() <= 1e-6 and (o["mel"][1, :24] > -5).any()
        assert (o["energy"][1, 24:] == 0).all() and (o["energy"][1, :23] > 0).all()
    ln = Mel("default", _lib.FS2_MEL_LN).run(wav, [5000, 8000], True)
    assert np.abs(ln["mel"][0, :20] - np.log(np.float32(g.clip))).max() <= 2e-6


def test_batch_invariance_bitwise():
    g = DEFAULT
    n = 20000
    x = R.signal("noise", n, 11)
    T, Te = R.frame_counts(n, g.hop)
    h = mel_handle("default", _lib.FS2_MEL_LOG10)

    def take(o, row):
        assert o["status"] == 0 and o["canaries"]
        return o["mel"][row, :T].copy(), o["energy"][row, :Te].copy()

    alone = take(h.run(x[None], [n], True), 0)
    others, wav, lens = batch_of((("ramp", 33000, 1), ("tone440", 9000, 2), ("noise", 31000, 3), ("noise", 500, 4)))
    for row in (0, 3):
        w, ll = wav.copy(), list(lens)
        w[row] = np.nan
        w[row, :n] = x
        ll[row] = n
        got = take(h.run(w, ll, True), row)
        assert np.array_equal(got[0].view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), alone[1].view(np.uint32)), row
    longer = np.full((1, 30001), np.nan, np.float32)
    longer[0, :n] = x
    for _ in range(2):  # inside a longer S, and that run twice
        got = take(h.run(longer, [n], True), 0)
        assert np.array_equal(got[0].view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), alone[1].view(np.uint32))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # a non-default stream: the same bits
        got = take(h.run(x[None], [n], True), 0)
    assert np.array_equal(got[0].view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), alone[1].view(np.uint32))


def test_peak_normalisation():
    """Seen on an MI355X: 9.1e-7 against float64 (model 8.3e-7), 2.2e-7 between normalising on the device and on the host."""
    g = DEFAULT
    n = 12000
    x = (0.37 * R.signal("noise", n, 21)).astype(np.float32)
    log, lin = mel_handle("default", _lib.FS2_MEL_LOG10), mel_handle("default", _lib.FS2_MEL_LINEAR)
    a, b = log.run(x[None], [n], True), log.run((2 * x)[None], [n], True)
    assert a["status"] == b["status"] == 0
    assert np.array_equal(a["mel"].view(np.uint32), b["mel"].view(np.uint32))  # a power-of-two scale is exact
    assert np.array_equal(a["energy"].view(np.uint32), b["energy"].view(np.uint32))
    xn = (x / np.abs(x).max()).astype(np.float32)
    on, off = lin.run(x[None], [n], True), lin.run(xn[None], [n], False)
    m64 = R.mel_ref(x, g, basis_of("default"), True)
    model = R.linear_figure(R.mel_chain(x, g, basis_of("default"), True), m64)
    figs = R.linear_figure(on["mel"][0], m64), R.linear_figure(on["mel"][0], off["mel"][0])
    print(f"peak normalisation: device vs float64 {figs[0]:.2e}, on vs off-on-normalised {figs[1]:.2e}, model {model:.2e}")
    assert model <= 1.5e-6 and figs[0] <= 2 * model and figs[1] <= 2 * model
    assert abs(float(np.abs(xn).max()) - 1.0) < 1e-6 and float(on["energy"].max()) <= 1.0


def test_energy():
    """against the float64 formula, held to 2x the float32 sequential-sum model (maxima over the case's frames).
    Seen on an MI355X: relative error 7.1e-8 / 9.3e-8 without / with peak normalisation (model 5.1e-7 / 3.6e-7)."""
    g = DEFAULT
    signals = tuple(("noise", n, n) for n in (1, 1023, 1024, 1025, 256 * 9))
    xs, wav, lens = batch_of(signals)
    h = mel_handle("default", _lib.FS2_MEL_LOG10)
    for pn in (False, True):
        o = h.run(wav, lens, pn)
        assert o["status"] == 0 and o["canaries"]
        dev = model = 0.0
        for i, x in enumerate(xs):
            Te = R.frame_counts(len(x), g.hop)[1]
            assert o["energy_frames"][i] == Te and (o["energy"][i, Te:] == 0).all()
            e64, e32 = R.energy_ref(x, g, pn), R.energy_chain(x, g, pn)
            assert (e64 > 0).all()
            dev = max(dev, float(np.abs(o["energy"][i, :Te] / e64 - 1).max()))
            model = max(model, float(np.abs(e32 / e64 - 1).max()))
        print(f"energy (peak_normalize {pn}): device {dev:.2e}, sequential float32 model {model:.2e}")
        assert dev <= 2 * model
    without = h.run(wav, lens, True, energy=False)  # energy = NULL is accepted and changes nothing else
    assert without["status"] == 0 and without["canaries"] and (without["energy"] == CANARY).all()
    assert np.array_equal(without["mel"].view(np.uint32), o["mel"].view(np.uint32))
    assert np.array_equal(without["energy_frames"], o["energy_frames"])


def test_segment_mean():
    """against the float64 restatement, held to 2x the float32 sequential-sum model.  Seen on an MI355X: 1.2e-7 / 3.2e-7 without /
    with stats - the model's own figures: the kernel sums a segment in the same order."""
    rng = np.random.RandomState(3)
    B, L, T = 3, 7, 12
    values = rng.standard_normal((B, T)).astype(np.float32) + 2.0
    frames = [12, 10, 12]
    durations = np.array([[2, 0, 3, 1, 0, 4, 2],    # sums to the frames it has, with zeros
                          [1, 2, 0, 3, 2, 0, 0],    # sums to fewer (8 of 10)
                          [3, 3, 0, 4, 5, 2, 1]],   # sums to more (18 of 12): one segment clipped, two empty after clipping
                         np.int32)
    vd = torch.from_numpy(values).to(DEV)
    canary = torch.full((B * L + SLACK,), CANARY, dtype=torch.float32, device=DEV)
    for mean, std in ((0.0, 1.0), (1.7, 0.6)):
        got = segment_mean(vd, torch.from_numpy(durations), torch.tensor(frames), mean, std).cpu().numpy()
        dev = model = 0.0
        for b in range(B):
            r64 = R.segment_mean_ref(values[b], frames[b], durations[b], mean, std)
            r32 = R.segment_mean_ref(values[b], frames[b], durations[b], mean, std, dtype=np.float32)
            dev, model = max(dev, float(np.abs(got[b] - r64).max())), max(model, float(np.abs(r32.astype(np.float64) - r64).max()))
        print(f"segment mean (mean {mean}, std {std}): device {dev:.2e}, sequential float32 model {model:.2e}")
        assert model > 0 and dev <= 2 * model
        assert got[2, 5] == got[2, 6] == np.float32((np.float32(1e-7) - np.float32(mean)) / np.float32(std))
    st = _lib.load().fs2_op_segment_mean(vd, None, torch.from_numpy(durations).to(DEV), B, T, L, 1e-7, 0, 1, canary,
                                         torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = canary.cpu().numpy()
    assert st == 0 and (out[B * L:] == CANARY).all()  # frames = NULL: every row has T frames
    assert np.allclose(out[:B * L].reshape(B, L)[2], R.segment_mean_ref(values[2], T, durations[2]), atol=1e-6)


def test_argument_errors_write_nothing():
    h = mel_handle("default", _lib.FS2_MEL_LOG10)
    x = R.signal("noise", 3000, 1)[None]
    ARG, NOMEM = _lib.FS2_ERR_ARG, _lib.FS2_ERR_NOMEM
    cases = [(dict(ws_short=1), NOMEM), (dict(T_max=3000 // 256), ARG), (dict(Te_max=11), ARG), (dict(null=("wav",)), ARG),
             (dict(null=("mel",)), ARG), (dict(null=("mel_frames",)), ARG), (dict(B=0), ARG)]
    for kw, want in cases:
        o = h.run(x, [3000], True, **kw)
        assert o["status"] == want and o["untouched"], (kw, o["status"])
        assert h.lib.fs2_mel_last_error(h.h) != b""
    ok = h.run(x, [3000], True, T_max=14, Te_max=13)  # larger output rows than the minimum are fine, and zero-filled
    assert ok["status"] == 0 and ok["canaries"] and (ok["mel"][0, 12:] == 0).all() and (ok["energy"][0, 12:] == 0).all()


def test_python_surface_and_training_targets():
    rng = np.random.RandomState(0)
    an = MelAnalyzer(device=DEV)
    wavs = [R.signal("noise", n, n) for n in (5000, 300, 12345)]
    out = an(wavs)
    assert sorted(out) == ["energy", "energy_lengths", "mel", "mel_lengths"]
    assert out["mel"].shape == (3, 1 + 12345 // 256, 80) and out["energy"].shape == (3, -(-12345 // 256))
    assert out["mel"].dtype == out["energy"].dtype == torch.float32 and out["mel_lengths"].dtype == out["energy_lengths"].dtype == torch.int32
    assert all(t.device == torch.device(DEV) for t in out.values())
    assert out["mel_lengths"].tolist() == [20, 2, 49] and out["energy_lengths"].tolist() == [20, 2, 49]
    same = an(torch.from_numpy(np.pad(wavs[0], (0, 100)))[None], lengths=[5000])  # a (B, S) host tensor with lengths
    assert torch.equal(same["mel"][0, :20], out["mel"][0, :20])
    # targets -> collate -> one training step at the train_small fixture's config
    from lightningfastspeech2_amd.config import Fs2Config
    from lightningfastspeech2_amd.frontend import collate
    from lightningfastspeech2_amd.training import Trainer
    from lightningfastspeech2_amd.weights import synth_state_dict
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_small.npz"))
    cfg = Fs2Config.from_json(str(z["config_json"]))
    skw = json.loads(str(z["synth_json"]))
    small = MelAnalyzer(n_mels=cfg.n_mels, mel_basis=slaney_mel_basis(cfg.sampling_rate, 1024, cfg.n_mels, 0, 8000),
                        hop_length=cfg.hop_length, device=DEV)
    phones = [row[row != 0] for row in z["in_phones"]]
    durs = [z["in_duration"][i][:len(p)] for i, p in enumerate(phones)]
    audio = [R.signal("noise", int(d.sum()) * cfg.hop_length + 100, 40 + i) for i, d in enumerate(durs)]
    for level in ("frame", "phone"):
        items = small.targets(audio, durs, stats=cfg.stats, energy_level=level)
        for i, it in enumerate(items):
            total = int(durs[i].sum())
            assert it["mel"].shape == (total, cfg.n_mels) and it["mel"].dtype == np.float32 and np.isfinite(it["mel"]).all()
            assert it["variances"]["energy"].shape == ((total,) if level == "frame" else (len(durs[i]),))
    items = small.targets(audio, durs, stats=cfg.stats)
    for i, it in enumerate(items):
        total = int(durs[i].sum())
        it["phones"], it["speaker"] = phones[i], z["in_speaker"][i]
        it["variances"] = {v: it["variances"]["energy"] if v == "energy" else rng.standard_normal(total).astype(np.float32)
                           for v in cfg.variances}
    batch = collate(items)
    assert batch["mel"].shape == (3, int(max(d.sum() for d in durs)), cfg.n_mels) and batch["variances_energy"].shape == batch["mel"].shape[:2]
    tr = Trainer(cfg, synth_state_dict(cfg, skw.pop("seed"), **skw), precision="fp32", **json.loads(str(z["hyper_json"])))
    losses = tr.training_step(batch)
    assert losses and all(np.isfinite(float(v)) for v in losses.values()), losses
