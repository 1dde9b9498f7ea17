"""CWT variance targets on the device (fs2_op_cwt_decompose, cwt_decompose, MelAnalyzer.items(transforms=...)) against
tests/_cwt_ref.py: ``CWT.decompose`` over SciPy 1.14's ``cwt`` / ``ricker``, restated.  The transform is not pinned against
scipy.signal.cwt's output (SciPy removed it); what is pinned is the definition in include/fs2.h, and tests/test_cwt_cpu.py holds
the restatement to the reference's own text.

Bars, per utterance of one ragged batch (counts around every scale's truncation point 10 w, both parities of M, the kernel's
512-output tiles, the cap of 4096; exact zeros in some rows, NaN in all padding), with e_dev = max |device - decompose_f64| and
e_ref = max |float32(decompose_ref) - decompose_f64|:
  spectrogram:  e_dev <= 2 e_ref + 4 ulp32(the utterance's spectrogram peak)   (2: the factor this project gives a sequential
                restatement's own error; the floor: rows so short that e_ref is near zero by chance)
  mean, std:    the same rule with a floor of 1 ulp32 of the value
  signal:       within 1 ulp32 of the float64 log;  original_signal: bit for bit;  everything at or past a count: exactly zero
Exact cases, bitwise batch invariance, refusals and the Python path end to end: bit for bit.

Seen on an MI355X (profiles/cwt.md): spectrogram e_dev / bar 0.42 ... 0.52 on 22 of the 34 utterances (both errors are the float32
rounding of `signal` carried through 1 / std, which the two paths share), 0.957 at the worst (n = 11: e_dev 3.06e-7, e_ref 1.45e-7); std at
most 0.958 (n = 22), mean 0.259; the tile-seam counts 0.44 ... 0.48.  The test prints every utterance's figures and adds the worst
ratios to the parity report.
"""
import functools

import numpy as np
import pytest
import torch

import _cwt_ref as R
from test_gpu_forward import _report  # a line of the parity report, where that file keeps it
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.analysis import MelAnalyzer, cwt_decompose, finish_contour, segment_mean, slaney_mel_basis

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY, SLACK = 777.0, 64
TILE = 512  # outputs one workgroup of cwt_decompose_kernel owns (stated in its comment)
KEYS = ("original", "signal", "spectrogram", "mean_std")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(values, counts, n_scales=R.N_SCALES, tau=R.TAU, null=(), B=None, S=None):
    """fs2_op_cwt_decompose straight through the C ABI (looked up in the library: every test here fails on one without it), every
    output buffer filled with a canary and with canaries behind it"""
    entry = _lib.load().fs2_op_cwt_decompose
    values = np.ascontiguousarray(values, np.float32)
    Bv, Sv = values.shape
    ns = max(1, n_scales)
    size = {"original": Bv * Sv, "signal": Bv * Sv, "spectrogram": Bv * Sv * ns, "mean_std": Bv * 2}
    bufs = {k: torch.full((size[k] + SLACK,), CANARY, dtype=torch.float32, device=DEV) for k in KEYS}
    a = {k: (None if k in null else v) for k, v in bufs.items()}
    cn = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    st = entry(torch.from_numpy(values).to(DEV), cn, Bv if B is None else B, Sv if S is None else S, n_scales, tau, a["original"], a["signal"],
               a["spectrogram"], a["mean_std"], torch.cuda.current_stream())
    torch.cuda.synchronize()
    host = {k: bufs[k].cpu().numpy() for k in KEYS}
    res = {"status": st, "original": host["original"][:Bv * Sv].reshape(Bv, Sv), "signal": host["signal"][:Bv * Sv].reshape(Bv, Sv),
           "spectrogram": host["spectrogram"][:Bv * Sv * ns].reshape(Bv, Sv, ns), "mean_std": host["mean_std"][:Bv * 2].reshape(Bv, 2)}
    res["canaries"] = bool(all((host[k][0 if k in null else size[k]:] == CANARY).all() for k in KEYS))
    res["untouched"] = bool(all((host[k] == CANARY).all() for k in KEYS))
    return res


def batch_of(rows, S=None, fill=np.nan):
    S = max(len(r) for r in rows) if S is None else S
    v = np.full((len(rows), S), fill, np.float32)
    for i, r in enumerate(rows):
        v[i, :len(r)] = r
    return v, [len(r) for r in rows]


@functools.lru_cache(maxsize=None)
def ragged():
    """the ragged batch through the device once, shared by the tests that look at it"""
    rows = R.ragged_rows()
    v, counts = batch_of(rows)
    assert v.shape == (len(R.COUNTS), 4096) and tuple(counts) == R.COUNTS
    o = run(v, counts)
    assert o["status"] == 0 and o["canaries"]
    return rows, counts, o


def check_spectrogram(dev, ref, f64, what):
    """the bar of the docstring on one utterance's (n, scales) spectrogram -> e_dev / bound"""
    truth = f64["spectrogram"]
    e_dev = float(np.abs(dev.astype(np.float64) - truth).max())
    e_ref = float(np.abs(ref["spectrogram"].astype(np.float32).astype(np.float64) - truth).max())
    bound = 2 * e_ref + 4 * R.ulp32(np.abs(truth).max())
    print(f"{what}: spectrogram e_dev {e_dev:.3e} e_ref {e_ref:.3e} peak {np.abs(truth).max():.3e} e_dev/bound {e_dev / bound if bound else 0.0:.3f}")
    assert np.isfinite(dev).all() and e_dev <= bound, (what, e_dev, e_ref, bound)
    return e_dev / bound if bound else 0.0


def test_accuracy_on_the_ragged_batch():
    rows, counts, o = ragged()
    refs = R.ragged_references()
    worst = {"spectrogram": 0.0, "mean": 0.0, "std": 0.0}
    for i, n in enumerate(counts):
        ref, f64 = refs[i]
        worst["spectrogram"] = max(worst["spectrogram"], check_spectrogram(o["spectrogram"][i, :n], ref, f64, f"n = {n}"))
        for j, k in enumerate(("mean", "std")):
            e_dev, e_ref = abs(float(o["mean_std"][i, j]) - float(f64[k])), abs(float(np.float32(ref[k])) - float(f64[k]))
            bound = 2 * e_ref + R.ulp32(f64[k])
            print(f"n = {n}: {k} e_dev {e_dev:.3e} e_ref {e_ref:.3e} e_dev/bound {e_dev / bound:.3f}")
            assert e_dev <= bound, (n, k, e_dev, e_ref, bound)
            worst[k] = max(worst[k], e_dev / bound)
        sig = o["signal"][i, :n]
        assert all(abs(float(s) - float(t)) <= R.ulp32(t) for s, t in zip(sig, f64["signal"])), n
        assert np.array_equal(bits(o["original"][i, :n]), bits(ref["original_signal"])), n
        assert (o["original"][i, :n] != 0).all() and ((rows[i] == 0) == (o["original"][i, :n] == np.float32(1e-7))).all()
        for k in ("original", "signal", "spectrogram"):  # +0 at and past the count (NaN was there in the input)
            assert not bits(o[k][i, n:]).any(), (n, k)
    print("worst e_dev / bound:", worst)
    _report(test="cwt_ragged_batch", utterances=len(counts), bar="2 e_ref + 4 ulp32(peak); mean, std: 2 e_ref + 1 ulp32",
            worst_ratio_to_bar={k: round(v, 4) for k, v in worst.items()})


def test_accuracy_at_the_kernels_own_seams():
    """counts on either side of the kernel's 512-output tiles (the ragged batch has every row's OUTPUTS cross them; here the counts do)"""
    rows = [R.contour(n, 300 + n) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1)]
    v, counts = batch_of(rows, S=3 * TILE)
    o = run(v, counts)
    assert o["status"] == 0 and o["canaries"]
    for i, n in enumerate(counts):
        check_spectrogram(o["spectrogram"][i, :n], R.decompose_ref(rows[i]), R.decompose_f64(rows[i]), f"n = {n}")
        assert not bits(o["spectrogram"][i, n:]).any() and not bits(o["signal"][i, n:]).any() and not bits(o["original"][i, n:]).any()


def test_exact_cases():
    const = np.full(700, 211.5, np.float32)
    one = np.array([97.0], np.float32)
    zeros = np.zeros(40, np.float32)  # every entry replaced by 1e-7: a constant row too
    v, counts = batch_of([const, one, R.contour(300, 5), zeros])
    o = run(v, counts)
    assert o["status"] == 0 and o["canaries"]
    for i, row in ((0, const), (1, one), (3, zeros)):
        n = len(row)
        assert o["mean_std"][i, 1] == 0.0 and not bits(o["spectrogram"][i]).any(), i  # std == 0, all-zero spectrogram: bitwise
        want = np.float32(np.log(np.float64(row[0] if row[0] else np.float32(1e-7))))
        assert o["mean_std"][i, 0] == want and (o["signal"][i, :n] == want).all(), i
    assert o["mean_std"][2, 1] > 0 and o["spectrogram"][2, :300].any()
    # n = 0: NaN mean_std, nothing else of the row written; the other row as if alone
    v, _ = batch_of([R.contour(20, 6), R.contour(33, 7)])
    o = run(v, [0, 33])
    alone = run(v[1:], [33])
    assert o["status"] == 0 and o["canaries"] and np.isnan(o["mean_std"][0]).all()
    assert all((o[k][0] == CANARY).all() for k in ("original", "signal", "spectrogram"))
    assert all(np.array_equal(bits(o[k][1]), bits(alone[k][0])) for k in KEYS)
    # counts are clamped to [0, S]; NULL counts mean full rows; NULL outputs are skipped
    full = R.contour(100, 8)[None]
    a, b, c = run(full, None), run(full, [100]), run(full, [5000])
    assert a["status"] == b["status"] == c["status"] == 0
    assert all(np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])) for k in KEYS)
    neg = run(np.concatenate([full, full]), [-3, 100])
    assert neg["status"] == 0 and np.isnan(neg["mean_std"][0]).all() and np.array_equal(bits(neg["spectrogram"][1]), bits(a["spectrogram"][0]))
    for null in (("spectrogram",), ("original", "signal"), ("mean_std",), KEYS):
        p = run(full, [100], null=null)
        assert p["status"] == 0 and p["canaries"]
        assert all(np.array_equal(bits(p[k]), bits(a[k])) for k in KEYS if k not in null), null


@pytest.mark.parametrize("n, p", [(200, 77), (201, 100), (2000, 1000)])
def test_an_impulse_like_row_is_centred_as_the_restatement_centres_it(n, p):
    """a flat contour with one outlier: x is a constant plus an impulse, so every scale shows its reversed, asymmetric wavelet about p.
    n = 200: M = 12 (even, untruncated), 23, 46, 91, 182, then 200 (even, truncated); 201: odd truncated; 2000: 363, 726 and 1451 untruncated"""
    v = np.full(n, 120.0, np.float32)
    v[p] = 480.0
    o = run(v[None], [n])
    assert o["status"] == 0 and o["canaries"]
    ref, f64 = R.decompose_ref(v), R.decompose_f64(v)
    check_spectrogram(o["spectrogram"][0], ref, f64, f"impulse n = {n}")
    got, want = o["spectrogram"][0].astype(np.float64), f64["spectrogram"]
    for i in range(R.N_SCALES):  # the truth moved by one output to either side is ten times further away than the truth, at every scale
        miss = min(np.abs(got[1:, i] - want[:-1, i]).max(), np.abs(got[:-1, i] - want[1:, i]).max())
        assert np.abs(got[:, i] - want[:, i]).max() < 0.1 * miss, i


def test_a_negative_sample_is_nan_in_its_own_utterance_only():
    rows = [np.array(r) for r in R.ragged_rows() if len(r) in (13, 182, 257, 726, 1451)]
    v, counts = batch_of(rows)
    clean = run(v, counts)
    v2 = v.copy()
    v2[2, 100] = -3.0
    o = run(v2, counts)
    assert clean["status"] == o["status"] == 0 and o["canaries"]
    n = counts[2]
    assert np.isnan(o["signal"][2, 100]) and np.isnan(o["mean_std"][2]).all() and np.isnan(o["spectrogram"][2, :n]).all()
    assert o["original"][2, 100] == -3.0
    others = np.delete(np.arange(n), 100)  # numpy's log is NaN at the negative entry alone
    assert np.array_equal(bits(o["signal"][2, others]), bits(clean["signal"][2, others])) and not bits(o["signal"][2, n:]).any()
    for i in (0, 1, 3, 4):
        assert all(np.array_equal(bits(o[k][i]), bits(clean[k][i])) for k in KEYS), i


def test_bitwise_batch_invariant():
    rows, counts, o = ragged()
    rs = np.random.RandomState(9)
    for i, n in enumerate(counts):  # each utterance alone, S = its own length
        a = run(np.array(rows[i])[None], [n])
        assert a["status"] == 0 and a["canaries"]
        assert np.array_equal(bits(a["mean_std"][0]), bits(o["mean_std"][i])), n
        assert all(np.array_equal(bits(a[k][0]), bits(o[k][i, :n])) for k in ("original", "signal", "spectrogram")), n
    # another S, another order, garbage (finite, negative, zero, huge) instead of NaN in the padding
    pick = [i for i, n in enumerate(counts) if n <= 1536][::-1]
    S = 1601
    v = (rs.standard_normal((len(pick), S)) * 1e6).astype(np.float32)
    v[:, ::7] = 0.0
    for j, i in enumerate(pick):
        v[j, :counts[i]] = rows[i]
    p = run(v, [counts[i] for i in pick])
    assert p["status"] == 0 and p["canaries"]
    for j, i in enumerate(pick):
        n = counts[i]
        assert np.array_equal(bits(p["mean_std"][j]), bits(o["mean_std"][i])), n
        for k in ("original", "signal", "spectrogram"):
            assert np.array_equal(bits(p[k][j, :n]), bits(o[k][i, :n])) and not bits(p[k][j, n:]).any(), (n, k)


def test_refusals_write_nothing():
    ARG, SHAPE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_SHAPE
    v = R.contour(64, 3)[None]
    assert run(v, [64])["status"] == 0
    big = np.full((1, 4097), 100.0, np.float32)
    cases = ((dict(values=big, counts=[4097]), SHAPE), (dict(values=big, counts=[10]), SHAPE), (dict(n_scales=0), ARG), (dict(n_scales=17), ARG),
             (dict(n_scales=-1), ARG), (dict(tau=0.0), ARG), (dict(tau=-R.TAU), ARG), (dict(tau=float("nan")), ARG), (dict(tau=float("inf")), ARG),
             (dict(B=0), ARG), (dict(S=0), ARG))
    for kw, want in cases:
        kw = dict(dict(values=v, counts=[64]), **kw)
        o = run(**kw)
        assert o["status"] == want and o["untouched"], (kw, o["status"])
    assert run(np.full((1, 4096), 100.0, np.float32), [7])["status"] == 0  # the cap itself runs
    for ns in (1, 16):  # the ends of 1 .. 16
        o = run(R.contour(300, 4)[None], [300], n_scales=ns)
        ref, f64 = R.decompose_ref(R.contour(300, 4), n_scales=ns), R.decompose_f64(R.contour(300, 4), n_scales=ns)
        assert o["status"] == 0 and o["canaries"] and o["spectrogram"].shape == (1, 300, ns)
        check_spectrogram(o["spectrogram"][0], ref, f64, f"n_scales = {ns}")
    with pytest.raises(ValueError, match="4096"):
        cwt_decompose(torch.ones(1, 4097, device=DEV))
    with pytest.raises(RuntimeError):
        cwt_decompose(torch.ones(1, 8, device=DEV), n_scales=17)


def test_python_surface_is_the_c_entry():
    rows = [R.contour(n, 20 + n) for n in (40, 513, 90)]
    rows[1][[3, 400]] = 0.0
    v, counts = batch_of(rows, fill=5.0)
    c = run(v, counts)
    p = cwt_decompose(torch.from_numpy(v).to(DEV), counts)
    assert sorted(p) == ["mean", "original_signal", "signal", "spectrogram", "std"] and p["spectrogram"].shape == (3, 513, 10)
    for k, want in (("original_signal", c["original"]), ("signal", c["signal"]), ("spectrogram", c["spectrogram"]), ("mean", c["mean_std"][:, 0]),
                    ("std", c["mean_std"][:, 1])):
        assert p[k].device.type == "cuda" and np.array_equal(bits(p[k].cpu().numpy()), bits(want)), k
    full = cwt_decompose(torch.from_numpy(v).to(DEV))  # counts=None: full rows, the filler included
    assert not np.array_equal(bits(full["mean"].cpu().numpy()), bits(c["mean_std"][:, 0]))
    import lightningfastspeech2_amd
    assert lightningfastspeech2_amd.cwt_decompose is cwt_decompose


def test_items_collate_training_step_on_the_class_default_configuration():
    """audio + durations + silence flags -> items(levels = phone x 3, transforms = cwt, none, none) -> collate -> Trainer.training_step on
    the tiny class-default configuration of tests/_train_variances.py; then transforms=None and "log" """
    import _targets_ref as T
    from _train_variances import case
    from lightningfastspeech2_amd.frontend import collate
    from lightningfastspeech2_amd.training import Trainer
    lengths = [7, 5]
    cfg, sd, synth = case(31, 2, 7, lengths, ("phone",) * 3, ("cwt", "none", "none"))
    assert cfg.is_cwt(0) and all(cfg.is_phone_level(i) for i in range(3)) and list(cfg.variances) == ["pitch", "energy", "snr"]
    hop, sr = cfg.hop_length, cfg.sampling_rate
    an = MelAnalyzer(sampling_rate=sr, n_mels=cfg.n_mels, mel_basis=slaney_mel_basis(sr, 1024, cfg.n_mels, 0, 8000), hop_length=hop, device=DEV,
                     wada_table=T.fixture()[0]["wada_table"])
    durs = [np.array([2, 3, 1, 4, 2, 3, 2], np.int64), np.array([3, 1, 2, 4, 3], np.int64)]  # no empty phone: log(log f0) stays finite
    silent = [np.array([1, 0, 0, 0, 0, 0, 0], bool), np.array([0, 0, 0, 0, 1], bool)]
    import _pitch_ref as P  # harmonic signals as tests/test_gpu_pitch.py builds them
    audio = []
    for i, (d, (f_a, f_b)) in enumerate(zip(durs, ((120.0, 180.0), (240.0, 180.0)))):  # two steady tones each: the phone means differ
        n, half = int(d.sum()) * hop + 100, int(d.sum()) * hop // 2
        audio.append(np.concatenate([P.tone(half, f_a, sr, 50 + i), P.tone(n - half, f_b, sr, 60 + i)]).astype(np.float32))
    names, levels = list(cfg.variances), ("phone",) * 3
    kw = dict(silent=silent, pitch="track", stats=cfg.stats, variances=names, levels=levels)
    items = an.items(audio, durs, transforms=("cwt", "none", "none"), **kw)
    plain = an.items(audio, durs, stats=None, **{k: v for k, v in kw.items() if k != "stats"})  # unnormalised, untransformed
    for i, it in enumerate(items):
        L, pv = len(durs[i]), it["variances"]["pitch"]
        assert list(pv) == ["signal", "original_signal", "spectrogram", "mean", "std"]
        assert pv["signal"].shape == (L,) and pv["original_signal"].shape == (L,) and pv["spectrogram"].shape == (L, 10)
        assert all(pv[k].dtype == np.float32 for k in pv) and pv["mean"].shape == () and pv["std"].shape == ()
        assert np.isfinite(pv["spectrogram"]).all() and pv["std"] >= 0 and (pv["original_signal"] > 50).all()
        # stats are not applied to a CWT variance: its input is the unnormalised phone means
        assert np.array_equal(bits(pv["original_signal"]), bits(plain[i]["variances"]["pitch"]))
        own = cwt_decompose(torch.from_numpy(pv["original_signal"])[None].to(DEV))
        assert np.array_equal(bits(own["spectrogram"][0].cpu().numpy()), bits(pv["spectrogram"]))
        assert np.array_equal(bits(own["signal"][0].cpu().numpy()), bits(pv["signal"])) and float(own["mean"][0]) == pv["mean"]
        ref = R.decompose_ref(pv["original_signal"])
        check_spectrogram(pv["spectrogram"], ref, R.decompose_f64(pv["original_signal"]), f"item {i}")
        it["phones"], it["speaker"] = synth["phones"][i][:L], synth["speaker"][i]
    batch = collate(items)
    assert batch["variances_pitch_signal"].shape == (2, 7) and batch["variances_pitch_spectrogram"].shape == (2, 7, 10)
    assert batch["variances_energy"].shape == (2, 7) and batch["variances_snr"].shape == (2, 7) and len(batch["variances_pitch_mean"]) == 2
    assert not batch["variances_pitch_spectrogram"][1, 5:].any()
    losses = Trainer(cfg, sd).training_step(batch)
    assert {"pitch_cwt", "total"} <= set(losses)
    assert all(np.isfinite(float(v)) for v in losses.values()), {k: float(v) for k, v in losses.items()}
    # transforms=None: the items as they were - the explicit "none"s and the call without the argument, bit for bit, and the pitch
    # what the primitives give with the stats
    none, default, explicit = an.items(audio, durs, transforms=None, **kw), an.items(audio, durs, **kw), an.items(audio, durs, transforms=("none",) * 3, **kw)
    f0 = an.pitch(audio)
    fin = finish_contour(f0["f0"], durs, silent, f0["f0_lengths"], zero_is_missing=True, all_missing_value=1e-7)
    dpad = np.zeros((2, 7), np.int32)
    for i, d in enumerate(durs):
        dpad[i, :len(d)] = d
    want = segment_mean(fin["values"], torch.from_numpy(dpad), fin["frames"], cfg.stats["pitch"]["mean"], cfg.stats["pitch"]["std"]).cpu().numpy()
    for i in range(2):
        for name in names:
            assert none[i]["variances"][name].dtype == np.float32 and none[i]["variances"][name].shape == (len(durs[i]),)
            assert np.array_equal(bits(none[i]["variances"][name]), bits(default[i]["variances"][name]))
            assert np.array_equal(bits(none[i]["variances"][name]), bits(explicit[i]["variances"][name]))
        assert np.array_equal(bits(none[i]["variances"]["pitch"]), bits(want[i, :len(durs[i])]))
        assert np.array_equal(bits(none[i]["mel"]), bits(items[i]["mel"]))
        for name in ("energy", "snr"):  # the untransformed neighbours of a CWT variance keep their stats
            assert np.array_equal(bits(none[i]["variances"][name]), bits(items[i]["variances"][name]))
    # "log": the log of the unnormalised variance, stats or none; priors are taken before any transform
    logged = an.items(audio, durs, transforms=("log", "none", "log"), priors=("pitch", "snr", "duration"), **kw)
    prior = an.items(audio, durs, priors=("pitch", "snr", "duration"), **kw)
    for i in range(2):
        for name in ("pitch", "snr"):
            raw = plain[i]["variances"][name]
            with np.errstate(invalid="ignore", divide="ignore"):
                want_log = np.log(raw.astype(np.float64))
            got = logged[i]["variances"][name]
            assert got.dtype == np.float32 and got.shape == raw.shape
            ok = np.isfinite(want_log)
            assert np.array_equal(np.isnan(got), np.isnan(want_log))
            assert all(abs(float(g) - float(w)) <= R.ulp32(w) for g, w in zip(got[ok], want_log[ok])), (i, name)
        assert np.isfinite(logged[i]["variances"]["pitch"]).all()
        assert np.array_equal(bits(logged[i]["variances"]["energy"]), bits(none[i]["variances"]["energy"]))
        assert logged[i]["priors"] == prior[i]["priors"] and all(np.isfinite(x) for x in prior[i]["priors"].values())
    # frame level: the finished contour over sum(d) frames
    frame = an.items(audio, durs, silent=silent, pitch="track", stats=cfg.stats, variances=("pitch",), levels=("frame",), transforms=("cwt",))
    for i, it in enumerate(frame):
        total = int(durs[i].sum())
        assert it["variances"]["pitch"]["spectrogram"].shape == (total, 10) and np.isfinite(it["variances"]["pitch"]["spectrogram"]).all()
        assert np.array_equal(bits(it["variances"]["pitch"]["original_signal"]), bits(fin["values"][i, :total].cpu().numpy()))
