"""Every kernel instantiation a HiFi-GAN generator can reach (tests/_voc_forms.py REACHABLE), run on the device.

A cell is (config, precision, resblock knob, LDS limit).  It synthesizes once and reads the engine's own launch record
(fs2_voc_last_launches): the record must be, launch for launch, what the host-side walk with the library's pickers predicts
(_voc_forms.plan), and must hold the instantiations the cell is in CELLS for.  Then the bars, all against the CPU oracle:
  fp32         every stage output within 1e-4 * (max|ref| + 1), the samples within 1e-3 (test_gpu_hifigan.test_stage_outputs_and_tile_seams)
  bf16 / fp16  rules (a), (b), (d) of test_gpu_hifigan_fp16._check with _voc16.generator_16bit under the cell's knob as the model:
               everything finite; the engine's (max, mean) error against the oracle at most twice the model's, stage by stage and on
               the samples; on bf16 samples at least half of it (the model describes the engine)
  all          the pad region exactly zero; every utterance alone bit-equal to itself inside the ragged batch.
Between runs of the engine only bit-equality is asserted: across LDS limits (tile heights only) and between knobs 1 and 4 (tile shapes
only).  Every measured tuple goes to the parity report (test names vocoder_forms_*); profiles/vocoder_forms.md keeps them."""
import functools
import threading

import numpy as np
import pytest
import torch

import _voc16
import _voc_forms as F
from test_gpu_forward import _report
from test_gpu_hifigan_fp16 import _seam, _valid   # V1's input with its cached oracle and models: computed once for both files
from lightningfastspeech2_amd.hifigan import HifiGan
from oracle import hifigan_cpu

pytestmark = pytest.mark.gpu
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}

# The smallest set of sweep cells (knob in _voc_forms.KNOBS x limit in _voc_forms.LIMITS) whose launches are the whole REACHABLE table: a
# greedy cover, most new instantiations first.  V1 reaches every compile-time stride at every height (its channels run 512 ... 32); the
# 1024-channel generator adds the runtime-stride build, the long-dilation one the half-height 8-wave tile in a 16-bit type.
CELLS = [
    ("v1", "fp32", 7, 150), ("v1", "bf16", 7, 76), ("v1", "fp16", 7, 76), ("v1", "bf16", 4, 24), ("v1", "fp16", 4, 24),
    ("v1", "fp32", 0, 76), ("v1", "bf16", 1, 150), ("v1", "fp16", 1, 150), ("v1", "bf16", 0, 52), ("v1", "fp16", 0, 52),
    ("v1", "fp32", 0, 52), ("wide", "fp32", 0, 0), ("wide", "bf16", 0, 0), ("wide", "bf16", 0, 150), ("wide", "fp16", 0, 0),
    ("wide", "fp16", 0, 150), ("long_dilation", "bf16", 1, 0), ("long_dilation", "fp16", 1, 0),
]
# (config, precision, knob) of the limit sweeps: conv by conv (every conv of every stage changes its tile) and the default, everywhere,
# and whatever else CELLS runs
GROUPS = sorted({(n, p, k) for n in F.CONFIGS for p in F.DTYPES for k in (0, 1)} | {c[:3] for c in CELLS})


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return _seam()[:4] if name == "v1" else F.inputs(name)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(wav, per-utterance stage outputs) of oracle/hifigan_cpu; V1's is test_gpu_hifigan_fp16._seam()'s"""
    if name == "v1":
        return _seam()[4]
    cfg, sd, mel, lengths = _inputs(name)
    return hifigan_cpu.synthesize(sd, cfg, mel, lengths, return_stages=True)


@functools.lru_cache(maxsize=None)
def _model(name, precision, knob):
    """the 16-bit-storage model under this resblock knob; the LDS limit is not its business (tile heights only)"""
    if name == "v1" and knob == 1:
        return _seam()[5 if precision == "bf16" else 6]
    cfg, sd, mel, lengths = _inputs(name)
    return _voc16.generator_16bit(sd, cfg, mel, lengths, TDT[precision], return_stages=True, knob=knob)


@functools.lru_cache(maxsize=None)
def _gen(name, precision):
    cfg, sd, _, _ = _inputs(name)
    return HifiGan(cfg, sd, precision=precision)


def _synth(name, precision, knob, limit):
    """one synthesize of the ragged batch under (knob, limit) -> wav, stage outputs (cpu), the engine's launch record"""
    cfg, _, mel, lengths = _inputs(name)
    g = _gen(name, precision)
    with F.knobs(knob, limit):
        wav = g.synthesize(mel, lengths).cpu()
        stages = [g.debug_stage(s).cpu() for s in range(len(cfg.upsample_rates) + 1)]
        record = g.last_launches()
    return wav, stages, record


@functools.lru_cache(maxsize=None)
def _run(cell):
    return _synth(*cell)


def _named(cell):
    """the instantiations this cell is in CELLS for: those of its predicted launches that no earlier cell has"""
    cfgs = {n: c[0] for n, c in F.CONFIGS.items()}
    before = set()
    for c in CELLS[:CELLS.index(cell)]:
        before |= {F.instantiation(l) for l in F.plan(cfgs[c[0]], *c[1:])}
    return {F.instantiation(l) for l in F.plan(cfgs[cell[0]], *cell[1:])} - before


def _bars(case, what, ref, model, got, scale, calibrate):
    """rules (a), (b), (d) for one 16-bit tensor: flat ref / model / engine over the same entries"""
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(model).all()), (case, what)                  # (d)
    em, eg = _voc16.errs(model, ref), _voc16.errs(got, ref)
    _report(test="vocoder_forms_16bit", case=f"{case}_{what}", scale=scale, model=[em[0] / scale, em[1] / scale], engine=[eg[0] / scale, eg[1] / scale])
    print(f"{case} {what}: model (max, mean) {em[0] / scale:.3e} {em[1] / scale:.3e}  engine {eg[0] / scale:.3e} {eg[1] / scale:.3e}")
    for i, stat in enumerate(("max", "mean")):
        assert eg[i] <= 2 * em[i], (case, what, stat, "engine vs model", eg, em)                                  # (b)
        if calibrate:
            assert eg[i] >= em[i] / 2, (case, what, stat, "calibration", eg, em)                                  # (a)


def _check_cell(cell, named):
    """one synthesize under the cell's knobs: the record (with `named` in it), the bars against the oracle, pads, batching"""
    name, precision, knob, limit = cell
    cfg, sd, mel, lengths = _inputs(name)
    L = lengths.tolist()
    wav, stages, record = _run(cell)
    case = "_".join(map(str, cell))
    # what ran: the engine's record against the host-side walk, and the instantiations this cell exists for
    assert record == F.plan(cfg, precision, knob, limit), case
    ran = {F.instantiation(l) for l in record}
    assert named <= ran and ran <= F.REACHABLE, (case, sorted(named - ran))
    # against the oracle
    ref_wav, ref_st = _oracle(name)
    ns = len(cfg.upsample_rates)
    if precision == "fp32":
        for s in range(ns + 1):
            up = int(np.prod(cfg.upsample_rates[:s])) if s else 1
            for b, n in enumerate(L):
                ref = ref_st[b][s]
                d = float((stages[s][b, :n * up] - ref).abs().max())
                bound = 1e-4 * (float(ref.abs().max()) + 1.0)
                _report(test="vocoder_forms_fp32", case=f"{case}_stage{s}_utt{b}", err=d, bound=bound)
                assert d <= bound, (case, s, b, d, bound)
        d = float((wav - ref_wav).abs().max())
        _report(test="vocoder_forms_fp32", case=f"{case}_wav", err=d, bound=1e-3)
        print(f"{case} wav: max {d:.3e}")
        assert d <= 1e-3, (case, d)
    else:
        m_wav, m_st = _model(name, precision, knob)
        for s in range(ns + 1):
            up = int(np.prod(cfg.upsample_rates[:s])) if s else 1
            pick = lambda per_utt: torch.cat([per_utt[b][s].reshape(-1) for b in range(len(L))])
            ref = pick(ref_st)
            _bars(case, f"stage{s}", ref, pick(m_st), _valid(stages[s], L, up), float(ref.abs().max()) + 1.0, False)
        _bars(case, "wav", _valid(ref_wav, L, cfg.hop), _valid(m_wav, L, cfg.hop), _valid(wav, L, cfg.hop), 1.0, precision == "bf16")
    # pads and batching
    g = _gen(name, precision)
    for b, n in enumerate(L):
        assert float(wav[b, n * cfg.hop:].abs().sum()) == 0.0, (case, b)
        with F.knobs(knob, limit):
            alone = g.synthesize(mel[b:b + 1, :n]).cpu()
        assert torch.equal(alone[0], wav[b, :n * cfg.hop]), (case, b)


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "-".join(map(str, c)))
def test_cell(cell):
    named = _named(cell)
    assert named   # a cell that adds nothing does not belong to the cover
    _check_cell(cell, named)


@pytest.mark.parametrize("precision", F.DTYPES)
@pytest.mark.parametrize("knob", [2, 9, 95])
def test_knobs_the_cover_does_not_need(knob, precision):
    """Knobs 2 (pairs only), 9 (raw streams between resident launches) and a percentage add no instantiation to the cover, but each is
    a launch sequence and - 9 - a stream layout of its own, which generator_16bit models: V1 under each, same record check, same bars.
    (Percentages up to 87 launch what knob 1 launches in every config here; under 95 two 128-channel pairs and the whole 64- and
    32-channel k = 3 blocks of the 16-bit types leave the 4-wave tile for the 8-wave one.)"""
    _check_cell(("v1", precision, knob, 0), set())


@pytest.mark.parametrize("precision", F.DTYPES)
@pytest.mark.parametrize("name", ["two_stage", "mid"])
def test_configs_the_cover_does_not_need(name, precision):
    """V1 reaches everything these two geometries reach, so no cell of the cover runs them; the limit sweeps and the knob 1 / 4 test
    below hold their runs bit-equal to the run under the default knobs - which this test holds to the oracle: same record check,
    same bars."""
    _check_cell((name, precision, 1, 0), set())


@pytest.mark.parametrize("name,precision,knob", GROUPS, ids=lambda v: str(v))
def test_lds_limit_changes_tile_heights_only(name, precision, knob):
    """Within one (config, precision, resblock knob) the LDS limit picks the conv tile heights and nothing else: every sample keeps its
    own arithmetic order whatever tile it falls in (what test_full_size_time_shift_equivariance relies on), so the samples and every
    stage output are the same bits under all limits - and under each of them the engine launched what the pickers said."""
    cfg = _inputs(name)[0]
    base = _synth(name, precision, knob, F.LIMITS[0])
    heights = set()
    for limit in F.LIMITS:
        wav, stages, record = base if limit == F.LIMITS[0] else _synth(name, precision, knob, limit)
        assert record == F.plan(cfg, precision, knob, limit), (name, precision, knob, limit)
        assert [l for l in record if l[0] == "resblock"] == [l for l in base[2] if l[0] == "resblock"]
        heights.add(tuple(l[2] for l in record if l[0] == "conv"))
        assert torch.equal(wav, base[0]), (name, precision, knob, limit, "wav")
        for s, (a, b) in enumerate(zip(stages, base[1])):
            assert torch.equal(a, b), (name, precision, knob, limit, "stage", s)
    assert len(heights) >= 3, heights   # the sweep did change tiles
    _report(test="vocoder_forms_limits", case=f"{name}_{precision}_knob{knob}", bit_exact=True, tilings=len(heights))


@pytest.mark.parametrize("precision", F.DTYPES)
@pytest.mark.parametrize("name", list(F.CONFIGS))
def test_knob_4_changes_tile_shapes_only(name, precision):
    """Knob 4 forbids the 4-wave resident tile: in these configs every pair and block that ran on one runs on a full-height 8-wave
    tile instead and nothing else changes - the same launches with the same streams stored activated - so the storage model is the
    same and the outputs are the same bits."""
    strip = lambda rec: [(l[0],) + (l[3:] if l[0] == "resblock" else l[2:]) for l in rec]
    one, four = _synth(name, precision, 1, 0), _synth(name, precision, 4, 0)
    assert strip(one[2]) == strip(four[2]), (name, precision)
    forms = lambda rec: {l[2] for l in rec if l[0] == "resblock"}
    if precision != "fp32":
        assert 408 in forms(one[2]) and 408 not in forms(four[2]) and 808 in forms(four[2])
    assert torch.equal(one[0], four[0]), (name, precision, "wav")
    for s, (a, b) in enumerate(zip(one[1], four[1])):
        assert torch.equal(a, b), (name, precision, "stage", s)
    _report(test="vocoder_forms_knob4", case=f"{name}_{precision}", bit_exact=True, forms_1=sorted(forms(one[2])), forms_4=sorted(forms(four[2])))


def test_knobs_belong_to_the_calling_thread():
    """include/fs2.h: fs2_voc_synthesize reads the switches of the thread that calls it.  Knob 0 on the main thread, knob 1 set by a
    worker thread for itself: the worker's synthesize runs resident launches, the main thread's - before and after - none."""
    name, precision = "two_stage", "bf16"
    cfg, _, mel, lengths = _inputs(name)
    g = _gen(name, precision)
    got = {}

    def worker():
        with F.knobs(1, 0):
            g.synthesize(mel, lengths)
            torch.cuda.synchronize()
            got["worker"] = g.last_launches()

    with F.knobs(0, 0):
        g.synthesize(mel, lengths)
        got["before"] = g.last_launches()
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        g.synthesize(mel, lengths)
        got["after"] = g.last_launches()
        want0 = F.plan(cfg, precision, 0, 0)   # leaves the defaults behind it: read last
    assert "worker" in got
    assert got["before"] == got["after"] == want0 and not any(l[0] == "resblock" for l in want0)
    assert got["worker"] == F.plan(cfg, precision, 1, 0) and any(l[0] == "resblock" for l in got["worker"])


def test_cells_cover_the_reachable_table():
    """the union of what the engine recorded over CELLS is the table tests/test_voc_forms_cpu.py pins, entry for entry"""
    ran = set()
    for cell in CELLS:
        ran |= {F.instantiation(l) for l in _run(cell)[2]}
    assert ran == F.REACHABLE, (sorted(F.REACHABLE - ran), sorted(ran - F.REACHABLE))
