"""The served forward (`-m gpu`): no debug taps, no forcing, both phases replayed as hipGraphs (fs2_set_graphs) - against a fresh
graphs-off engine bit for bit, and against the CPU oracle under the served forward's own decisions.

Every other oracle test sets debug mode or forces durations / buckets, and both turn off what the served path runs: the graph replay
(run_phase) and, at H = 256, the variance embedding riding in the predictor launch (variance_stage's tail).  Here the matrix is
{dense C2, depth-wise ref-default} x variance layouts (frame / phone level, CWT, priors, one non-256 width) x precisions, and per cell
the ways a served engine is driven: replays on the same input tensors, new data in the same tensors, a shape change with the
zero-duration guard firing and back, a kernel switch under graphs, pipelines, a clone made after capture, and a caller workspace of
exactly the reported size."""

import numpy as np
import pytest
import torch

from _teacher import teacher_targets
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.config import Fs2Config, preset
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
from oracle import oracle_cpu
from test_gpu_forward import BF16_ENC_MAX, BF16_MEL_MAX, BF16_MEL_MEAN, MEL_TOL_FP32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CWT_PITCH = {"pitch": {"min": 0.2, "max": 5.0, "mean": 0.1, "std": 1.5}, "energy": {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0},
             "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0}}
CWT_PITCH_ENERGY = {**CWT_PITCH, "energy": {"min": 0.3, "max": 4.0, "mean": 0.0, "std": 1.0}}
PRIORS = {"pitch": {"min": -2.0, "max": 2.5, "mean": 0.1, "std": 1.5}, "energy": {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0},
          "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0}, "pitch_prior": {"min": -1.0, "max": 1.0},
          "duration_prior": {"min": 0.0, "max": 5.0}}
LAYOUTS = {
    "frame": {},                                                        # all frame level: the control
    "phone1": dict(variance_levels=["phone", "frame", "frame"]),        # odd number of phone-level embeddings
    "phone2": dict(variance_levels=["phone", "frame", "phone"]),
    "phone3": dict(variance_levels=["phone", "phone", "phone"]),        # no frame-level variance left: pe + spk as their own launch
    "phone_cwt_energy": dict(variance_levels=["phone", "phone", "frame"], variance_transforms=["cwt", "none", "none"], stats=CWT_PITCH),
    "frame_cwt": dict(variance_transforms=["cwt", "none", "none"], stats=CWT_PITCH),  # the reference's class default
    "phone_cwt2": dict(variance_levels=["phone", "phone", "frame"], variance_transforms=["cwt", "cwt", "none"], stats=CWT_PITCH_ENERGY),
    "priors": dict(variance_levels=["phone", "frame", "frame"], priors=["pitch", "duration"], stats=PRIORS),
    "h128": dict(variance_levels=["phone", "frame", "frame"], encoder_hidden=128, decoder_hidden=128, variance_filter_size=128,
                 duration_filter_size=128, encoder_conv_filter_size=512, decoder_conv_filter_size=512),  # the tail is not fused
}
CELLS = [(b, lay, prec) for b in ("c2", "ref-default") for lay in LAYOUTS for prec in ("bf16", "fp32x3", "mixed3")]
CELLS += [(b, "phone1", prec) for b in ("c2", "ref-default") for prec in ("fp32", "mixed")]
VARIANTS = ["replay", "new_data", "guard_shape", "knob", "pipelines", "clone", "exact_workspace", "oracle"]
B, L, LG = 3, 120, 16


def _cfg(base, layout):
    return Fs2Config(**{**preset(base).to_dict(), **LAYOUTS[layout]})


def _model(cfg, sd, precision, graphs):
    from lightningfastspeech2_amd.model import FastSpeech2
    m = FastSpeech2(cfg, sd, precision=precision, device=DEV)
    m.engine.set_graphs(graphs)
    return m


def _flat(out, prefix=""):
    res = {}
    for k, v in out.items():
        if isinstance(v, dict):
            res.update(_flat(v, f"{prefix}{k}."))
        elif isinstance(v, torch.Tensor):
            res[prefix + k] = v.detach().cpu().clone()
    return res


def _same(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, f"{what}: {bad} differ from the graphs-off engine"


class Served:
    """An engine driven as a server drives it: the same device input tensors, one output set per (B, L, T), kept."""

    def __init__(self, engine):
        self.e, self.outs = engine, {}

    def __call__(self, bt):
        e = self.e
        Bq, Lq = bt["phones"].shape
        T = e.encode(bt["phones"], bt["speaker"], None, bt.get("priors"))
        outs = self.outs.setdefault((Bq, Lq, T), e.alloc_outputs(Bq, Lq, T))
        e.decode(outputs=outs)
        torch.cuda.synchronize()
        res = _flat(outs)
        res["guard"] = torch.from_numpy(e.totals()[1].copy())
        return res


class Cell:
    """Weights, the three batches and the graphs-off engine's outputs of one (base, layout, precision)."""

    def __init__(self, base, layout, prec):
        self.base, self.layout, self.prec = base, layout, prec
        self.cfg = cfg = _cfg(base, layout)
        self.sd = synth_state_dict(cfg, 11, randomize_norm=True, duration_bias=1.3)
        self.ref = _model(cfg, self.sd, prec, graphs=False)
        spk = synth_inputs(cfg, 1, 1, seed=5)["speaker"][0]
        pri = np.array([[0.4], [2.0]], np.float32)[: len(cfg.priors)]  # one value per prior for every utterance (the probe's too)
        # one-phone utterances whose duration is a clear decision, found by probe batches: every phone id at position 0 of an
        # (Lc)-wide row - the context the utterance sees below (the reference's convolutions read the pad rows too) - under given
        # speakers.  A one-phone utterance whose duration rounds to 0 trips the guard: its speaker is searched among scaled random
        # directions too, and where none gets there the duration head's bias is lowered until one does.
        def probe(Lc, spks):
            n, ns = cfg.n_phones - 1, len(spks)
            ph = torch.zeros(ns, n, Lc, dtype=torch.int64)
            ph[:, :, 0] = torch.arange(1, cfg.n_phones)
            bt = {"phones": ph.reshape(ns * n, Lc).to(DEV),
                  "speaker": torch.from_numpy(np.repeat(np.stack(spks), n, axis=0)).to(DEV).contiguous()}
            if cfg.priors:
                bt["priors"] = torch.from_numpy(np.repeat(pri, ns * n, axis=1)).to(DEV).contiguous()
            return Served(self.ref.engine)(bt)["duration_prediction"][:, 0].reshape(ns, n)
        rs = np.random.RandomState(7)
        dirs = rs.standard_normal((24, spk.shape[0])).astype(np.float32)
        spks = [spk] + [(d / np.linalg.norm(d) * k).astype(np.float32) for d in dirs for k in (1.0, 4.0, 16.0)]
        dp_g = probe(LG, spks)
        if float(dp_g.min()) > np.log(1.5) - 0.2:  # lower the duration head's bias (a shift of every log-duration) until one rounds to 0
            bias = round(1.3 - (float(dp_g.min()) - np.log(1.5) + 0.25), 3)
            self.sd = synth_state_dict(cfg, 11, randomize_norm=True, duration_bias=bias)
            self.ref = _model(cfg, self.sd, prec, graphs=False)
            dp_g = probe(LG, spks)
        dp_a = probe(L, [spk])[0]
        long_ph = int(torch.argmax(dp_a)) + 1
        i = int(torch.argmin(dp_g))
        gspk, short_ph = spks[i // dp_g.shape[1]], i % dp_g.shape[1] + 1
        assert float(dp_g.min()) < np.log(1.5) - 0.1 and float(dp_a.max()) > np.log(1.5) + 0.1, \
            ("no clear one-phone decisions in the probes", float(dp_g.min()), float(dp_a.max()))

        def batch(seed, lengths, Lb, one_phone=None):
            inp = synth_inputs(cfg, B, Lb, seed=seed, lengths=lengths)
            if one_phone is not None:  # utterance i: the probe's phone under the probe's speaker
                i, ph, sv = one_phone
                inp["phones"][i, 0], inp["speaker"][i] = ph, sv
            bt = {"phones": inp["phones"], "speaker": inp["speaker"]}
            if cfg.priors:
                bt["priors"] = np.repeat(pri, B, axis=1)
            return bt
        self.host = {"A": batch(21, [L, 57, 1], L, (2, long_ph, spk)),           # ragged, a one-phone utterance, no guard
                     "B": batch(22, [83, L, 9], L),                              # same shape, different durations
                     "G": batch(23, [LG, 1, 11], LG, (1, short_ph, gspk))}      # another shape: the guard fires for utterance 1
        self.want = {k: Served(self.ref.engine)(self.dev(k)) for k in self.host}
        ta, tb, tg = (self.want[k]["mel"].shape[1] for k in "ABG")
        assert ta != tb and tg > 0, "the batches must differ in T"
        assert self.want["A"]["guard"].sum() == 0 and self.want["B"]["guard"].sum() == 0
        assert self.want["G"]["guard"].tolist() == [0, 1, 0]

    def dev(self, k):
        """A new device copy of batch k (the Served format: priors as one (n_priors, B) tensor)."""
        h = self.host[k]
        bt = {"phones": torch.from_numpy(h["phones"]).to(DEV), "speaker": torch.from_numpy(h["speaker"]).to(DEV)}
        if "priors" in h:
            bt["priors"] = torch.from_numpy(h["priors"]).to(DEV).contiguous()
        return bt

    def model_batch(self, k, device=True):
        """Batch k as FastSpeech2.forward takes it (priors_<p> keys); device tensors or pinned host tensors."""
        h = self.host[k]
        t = lambda a: torch.from_numpy(a).to(DEV) if device else torch.from_numpy(a).pin_memory()
        bt = {"phones": t(h["phones"]), "speaker": t(h["speaker"])}
        for i, pr in enumerate(self.cfg.priors):
            bt[f"priors_{pr}"] = torch.from_numpy(h["priors"][i].copy())
        return bt

    def served(self):
        """A served model: the cell's graphs-on engine itself the first time, then fresh replicas over its weights (fs2_clone: own
        workspace, host state and graph cache) - the engines a pipeline runs."""
        if not hasattr(self, "_srv"):
            self._srv = _model(self.cfg, self.sd, self.prec, graphs=True)
            return self._srv
        return self._srv.replicate()

    def replays(self, n):
        """Phase replays of n forwards of one batch on a fresh engine: the decode phase from the second forward on (the first one grows
        the torch workspace to this T), the encode phase from the third (its scratch address changed at that growth) - unless priors,
        a one-shot pointer of the call, keep it plain"""
        return (n - 1) + (0 if self.cfg.priors else n - 2)


_cell = {}


def _get_cell(base, layout, prec):
    key = (base, layout, prec)
    if key not in _cell:
        _cell.clear()
        torch.cuda.empty_cache()
        _cell[key] = Cell(base, layout, prec)
    return _cell[key]


def _ids(c):
    return "-".join(c)


def _applies(cell, variant):
    cfg = _cfg(*cell[:2])
    return variant != "oracle" or not any(cfg.is_cwt(i) for i in range(len(cfg.variances)))  # a CWT variance is teacher-forced with
    # its raw signal, which the forward does not return


@pytest.mark.parametrize("cell,variant", [(c, v) for c in CELLS for v in VARIANTS if _applies(c, v)],
                         ids=[f"{_ids(c)}-{v}" for c in CELLS for v in VARIANTS if _applies(c, v)])
def test_served_path(cell, variant):
    c = _get_cell(*cell)
    globals()[f"_check_{variant}"](c)


def _check_replay(c):
    """Graphs on, six forwards on the same device tensors: first sight plain, second captured, then replays."""
    m = c.served()
    s, a = Served(m.engine), c.dev("A")
    n0 = m.engine.graph_replays()
    for it in range(6):
        _same(s(a), c.want["A"], f"replay forward {it}")
    assert m.engine.graph_replays() - n0 == c.replays(6)


def _check_new_data(c):
    """The same device tensors overwritten in place with another batch (another T): the encode graph replays on the new contents."""
    m = c.served()
    s, a = Served(m.engine), c.dev("A")
    src = {k: c.dev(k) for k in "AB"}
    n0 = m.engine.graph_replays()
    seq = "AABBABAB"
    for it, k in enumerate(seq):
        for name, t in a.items():
            t.copy_(src[k][name])
        _same(s(a), c.want[k], f"forward {it} ({k})")
    assert m.engine.graph_replays() - n0 >= (0 if c.cfg.priors else len(seq) - 2), "the encode phase never replayed"


def _check_guard_shape(c):
    """Replays, a batch of another shape in which the zero-duration guard fires (its flags come back through the captured pinned
    copy), and back."""
    m = c.served()
    s, a, g = Served(m.engine), c.dev("A"), c.dev("G")
    n0 = m.engine.graph_replays()
    for it, k in enumerate("AAAGGGAGAG"):
        got = s(a if k == "A" else g)
        _same(got, c.want[k], f"forward {it} ({k})")
        tot, grd = m.engine.totals()
        assert grd.tolist() == c.want[k]["guard"].tolist()
        assert tot.max() == c.want[k]["mel"].shape[1]
    # A as in replay (3 forwards), G's signatures are new (its workspace fits in A's), then every later forward replays both phases
    assert m.engine.graph_replays() - n0 >= c.replays(3) + (6 if c.cfg.priors else 12)


def _check_knob(c):
    """set_tuning(1320) / (1321) (the embedding in the predictor launch off / on) under graphs: each matches its own eager output."""
    c.ref.engine.set_tuning(1320)
    try:
        want1320 = Served(c.ref.engine)(c.dev("A"))
    finally:
        c.ref.engine.set_tuning(1321)
    m = c.served()
    s, a = Served(m.engine), c.dev("A")
    for knob, want in ((1320, want1320), (1321, c.want["A"]), (1320, want1320), (1321, c.want["A"])):
        m.engine.set_tuning(knob)
        for it in range(3):
            _same(s(a), want, f"knob {knob} forward {it}")


def _check_pipelines(c):
    """pipeline(2) with device inputs and pipeline(3, host_outputs) with pinned host inputs, graphs on, two batches mixed: results
    in submission order equal the eager forward's."""
    want = {k: _flat(c.ref(c.model_batch(k), inference=True)) for k in "AB"}
    order = "ABAABBAB"
    m = c.served()
    dev = {k: c.model_batch(k) for k in "AB"}
    pipe = m.pipeline(2)
    try:
        warm = []  # each replica's torch workspace grows to both batches' sizes first (a growth is a new signature)
        for k in "AABB":
            warm += [_flat(o) for o in pipe.submit(dev[k])]
        warm += [_flat(o) for o in pipe.drain()]
        n0 = [r.engine.graph_replays() for r in pipe.models]
        got = []
        for k in order:
            got += [_flat(o) for o in pipe.submit(dev[k])]
        got += [_flat(o) for o in pipe.drain()]
        grew = [r.engine.graph_replays() - n for r, n in zip(pipe.models, n0)]
    finally:
        pipe.close()
    assert len(warm) == 4 and len(got) == len(order)
    for i, (k, o) in enumerate(zip("AABB" + order, warm + got)):
        _same(o, want[k], f"pipeline(2) result {i} ({k})")
    assert c.cfg.priors or all(gr > 0 for gr in grew), grew  # (with priors only a repeated output set replays: the decode phase)
    host = {k: c.model_batch(k, device=False) for k in "AB"}
    pipe = m.pipeline(3, host_outputs=("mel", "tgt_mask"))
    try:
        got = []
        for k in order:
            got += [_flat(o) for o in pipe.submit(host[k])]  # _flat copies: a host output is a view of a ring slot
        got += [_flat(o) for o in pipe.drain()]
    finally:
        pipe.close()
    assert len(got) == len(order)
    for i, (k, o) in enumerate(zip(order, got)):
        _same(o, want[k], f"pipeline(3, host_outputs) result {i} ({k})")


def _check_clone(c):
    """An engine cloned from one that has captured graphs gives the eager outputs on its first and later calls."""
    m = c.served()
    s, a = Served(m.engine), c.dev("A")
    for _ in range(4):
        s(a)
    for make in (lambda: m.engine.clone(), lambda: m.replicate().engine):
        e = make()
        s2 = Served(e)
        n0 = e.graph_replays()
        for it in range(4):
            _same(s2(a), c.want["A"], f"clone forward {it}")
        assert e.graph_replays() - n0 == c.replays(4)
    _same(s(a), c.want["A"], "the source after cloning")


def _check_exact_workspace(c):
    """fs2_workspace_bytes is enough: the caller's buffers are exactly the reported sizes (no allocator slack) - the encode phase's
    scratch for T = 0, then the decode phase's for this batch's T - and the forward replays under graphs in them."""
    m = c.served()
    e = m.engine.clone()
    e.torch_workspace = False  # the buffers below are the only workspace it has
    lib, h = e.lib, e.handle
    bufs = {}

    def ws(what, persist, scratch):
        _lib.check(lib.fs2_set_workspace(h, persist, persist.numel(), scratch, scratch.numel()), h, what)
    for k in ("A", "G", "A", "A", "G", "A"):
        bt = c.dev(k) if k not in bufs else bufs[k][0]
        Bq, Lq = bt["phones"].shape
        T = c.want[k]["mel"].shape[1]
        if k not in bufs:
            pb, sb_enc = e.workspace_bytes(Bq, Lq, 0)
            _, sb_dec = e.workspace_bytes(Bq, Lq, T)
            bufs[k] = (bt, torch.empty(pb, dtype=torch.uint8, device=DEV), torch.empty(sb_enc, dtype=torch.uint8, device=DEV),
                       torch.empty(sb_dec, dtype=torch.uint8, device=DEV), {})
        bt, persist, s_enc, s_dec, outs = bufs[k]
        ws("set_workspace(encode)", persist, s_enc)
        assert e.encode(bt["phones"], bt["speaker"], None, bt.get("priors")) == T
        ws("set_workspace(decode)", persist, s_dec)
        o = outs.setdefault("o", e.alloc_outputs(Bq, Lq, T))
        e.decode(outputs=o)
        torch.cuda.synchronize()
        got = _flat(o)
        got["guard"] = torch.from_numpy(e.totals()[1].copy())
        _same(got, c.want[k], f"exact workspace ({k})")
    assert e.graph_replays() > 0


def _check_oracle(c):
    """The served output at the fourth replayed forward against the CPU oracle under the served forward's own decisions (durations,
    every variance bucket): the oracle's predictions under those decisions match the GPU's, and so does the mel."""
    m = c.served()
    s, a = Served(m.engine), c.dev("A")
    n0 = m.engine.graph_replays()
    for _ in range(6):
        out = s(a)
    assert m.engine.graph_replays() - n0 == c.replays(6)
    assert out["guard"].sum() == 0
    h = c.host["A"]
    pri = {f"priors_{pr}": h["priors"][i] for i, pr in enumerate(c.cfg.priors)}
    ref = oracle_cpu.forward(c.sd, c.cfg, h["phones"], h["speaker"], priors=pri, teacher_targets=teacher_targets(c.cfg, out))
    split = c.prec != "bf16"   # fp32 / split-arithmetic front: every decision's input is fp32-grade
    fp32_dec = c.prec in ("fp32", "fp32x3")
    tol_pred = MEL_TOL_FP32 if split else BF16_ENC_MAX
    assert torch.equal(out["tgt_mask"], ref["tgt_mask"]) and torch.equal(out["src_mask"], ref["src_mask"])
    errs = {k: float((out[k] - ref[k]).abs().max()) for k in ["duration_prediction"] + [f"variances_{v}" for v in c.cfg.variances]}
    mel_max = float((out["mel"] - ref["mel"]).abs().max())
    mel_mean = float((out["mel"] - ref["mel"]).abs().mean())
    for k, err in errs.items():
        assert err <= tol_pred, (k, err, tol_pred, errs)
    if fp32_dec:
        assert mel_max <= MEL_TOL_FP32, (mel_max, errs)
    else:
        assert mel_max <= BF16_MEL_MAX and mel_mean <= BF16_MEL_MEAN, (mel_max, mel_mean, errs)


@pytest.mark.parametrize("prec", ["bf16", "fp32x3", "mixed3", "fp32", "mixed"])
def test_embedding_tail_runs_where_expected(prec):
    """The odd-parity cells are not vacuous: at H = 256 the bf16 and split-arithmetic engines embed every non-CWT variance inside its
    predictor launch (one stand-alone bucket/embedding launch fewer per variance than with knob 1320); plain fp32 fronts never do."""
    c = _get_cell("c2", "phone1", prec)
    e = c.ref.engine.clone()
    rowops = 3  # FS2_K_ROWOPS: the stand-alone bucket/embedding launches are counted here
    a = c.dev("A")
    n = {}
    try:
        for knob in (1321, 1320):
            e.set_tuning(knob)
            e.profile_enable(rowops, True)
            _same(Served(e)(a), c.want["A"], f"knob {knob} with profiling")
            n[knob] = e.profile_read(rowops)["launches"]
    finally:
        e.profile_enable(rowops, False)
    tails = n[1320] - n[1321]
    assert tails == (len(c.cfg.variances) if prec in ("bf16", "fp32x3", "mixed3") else 0), (prec, n)
