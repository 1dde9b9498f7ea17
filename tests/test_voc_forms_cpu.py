"""Which vocoder kernel instantiations a generator can reach, decided on the host (no device): the library's two pickers
(fs2_op_vocoder_resblock_form, fs2_op_vocoder_conv_tile) against the tests' own restatement (_voc16.resident_form) and against two
pinned tables - what the HiFi-GAN V1 family reaches under every value of the two knobs, and what the launchers can name but no such
geometry reaches.  tests/test_gpu_hifigan_forms.py runs every entry of the first table on the device."""
import ctypes as C
import os

import pytest

import _voc16
import _voc_forms as F
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.hifigan import decode_launch

PCT = tuple(range(50, 101))
ALL_KNOBS = (0, 1, 2, 4, 7, 9) + PCT

REACHABLE, UNREACHABLE = F.REACHABLE, F.UNREACHABLE   # the two pinned tables (tests/_voc_forms.py)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_resident_restates_the_exported_picker(lib):
    """_voc16.resident_form - what generator_16bit takes its stream layout from - against voc_resblock_mi16 itself: every width the
    engine packs (and 256, which it does not), odd taps 1..13, one pair at dilations 1..9 and the dilation triples the tests use, every
    knob value, 2- and 4-byte storage"""
    triples = {tuple(ds) for cfg, *_ in F.CONFIGS.values() for ds in cfg.resblock_dilation_sizes} | {(1, 3, 5), (1, 2, 3), (1, 3, 9)}
    dils = [[d] for d in range(1, 10)] + sorted(list(t) for t in triples)
    seen = set()
    for knob in ALL_KNOBS:
        with F.knobs(knob, 0):
            for precision, esz in (("fp32", 4), ("bf16", 2), ("fp16", 2)):
                for c in (32, 64, 128, 256):
                    for taps in range(1, 14, 2):
                        for ds in dils:
                            got = F.resblock_form(lib, precision, c, taps, ds)
                            assert got == _voc16.resident_form(c, taps, ds, knob, esz), (knob, precision, c, taps, ds)
                            assert _voc16.resident(c, taps, ds, knob, esz) == (got != 0)
                            seen.add(got)
    assert seen == {0, 408, 808, 804}   # the grid exercises every branch of the rule


def test_pickers_read_the_calling_threads_knobs_and_refuse_bad_arguments(lib):
    d = (C.c_int32 * 3)(1, 3, 5)
    assert lib.fs2_op_vocoder_resblock_form(_lib.FS2_BF16, 64, 3, d, 3) == 408       # the defaults: knob 1
    with F.knobs(4, 0):
        assert lib.fs2_op_vocoder_resblock_form(_lib.FS2_BF16, 64, 3, d, 3) == 808
    with F.knobs(2, 0):
        assert lib.fs2_op_vocoder_resblock_form(_lib.FS2_BF16, 64, 3, d, 3) == 0 and lib.fs2_op_vocoder_resblock_form(_lib.FS2_BF16, 64, 3, d, 1) == 408
    assert lib.fs2_op_vocoder_resblock_form(_lib.FS2_BF16, 64, 3, d, 3) == 408       # the context restored them
    for bad in ((_lib.FS2_MIXED, 64, 3, d, 3), (_lib.FS2_BF16, 64, 3, d, 2), (_lib.FS2_BF16, 64, 3, None, 1), (_lib.FS2_BF16, 64, 0, d, 1),
                (_lib.FS2_BF16, 64, 3, (C.c_int32 * 3)(1, 0, 5), 3)):
        assert lib.fs2_op_vocoder_resblock_form(*bad) < 0, bad[:3]
    pad = C.c_int32(0)
    # V1's 256-channel stage: a 128-row tile under the heuristic's 110 KiB, a 224-row one with the whole 150
    assert lib.fs2_op_vocoder_conv_tile(_lib.FS2_BF16, 256, 256, 11, 5, 0, 0, C.byref(pad)) == 8 and pad.value == 256
    with F.knobs(1, 150):
        assert lib.fs2_op_vocoder_conv_tile(_lib.FS2_BF16, 256, 256, 11, 5, 0, 0, None) == 14
    with F.knobs(1, 1):   # nothing fits 1 KiB: the shortest tile is taken up to the hardware's 150 KiB
        assert lib.fs2_op_vocoder_conv_tile(_lib.FS2_BF16, 256, 256, 11, 5, 0, 0, None) == 2
    assert lib.fs2_op_vocoder_conv_tile(_lib.FS2_F32, 512, 80, 7, 1, 0, 0, C.byref(pad)) == 8 and pad.value == 128    # conv_pre: 80 mel bins
    assert lib.fs2_op_vocoder_conv_tile(_lib.FS2_F16, 1024, 1024, 2, 1, 1, 0, C.byref(pad)) == 2 and pad.value == 1024
    assert lib.fs2_op_vocoder_conv_tile(_lib.FS2_F16, 1, 32, 7, 1, 0, 1, C.byref(pad)) == 8 and pad.value == 32       # conv_post: one wave column, 8 wave rows
    for bad in ((_lib.FS2_MIXED, 256, 256, 3, 1, 0, 0, None), (_lib.FS2_BF16, 48, 256, 3, 1, 0, 0, None), (_lib.FS2_BF16, 256, 0, 3, 1, 0, 0, None),
                (_lib.FS2_BF16, 256, 256, 3, 0, 0, 0, None)):
        assert lib.fs2_op_vocoder_conv_tile(*bad) < 0, bad[:5]


def test_up_taps_is_the_engines_tap_window_rule():
    """k = 2s: two of three taps per phase (two windows); k = 3s: all three; k = s: one"""
    assert [F.up_taps(k, s) for k, s in ((16, 8), (4, 2), (8, 4), (12, 4), (6, 2), (2, 2), (8, 8))] == \
        [(2, True), (2, True), (2, True), (3, False), (3, False), (1, False), (1, False)]


def test_decode_launch():
    assert decode_launch(_lib.FS2_F16 << 1 | 14 << 4 | 512 << 8 | 1 << 19) == ("conv", "fp16", 14, 512, False, True, False)
    assert decode_launch(_lib.FS2_F32 << 1 | 2 << 4 | 1 << 18 | 1 << 20) == ("conv", "fp32", 2, 0, True, False, True)
    assert decode_launch(1 | _lib.FS2_BF16 << 1 | 808 << 4 | 128 << 14 | 1 << 22 | 1 << 24) == ("resblock", "bf16", 808, 128, 1, True, False)
    assert decode_launch(1 | _lib.FS2_F32 << 1 | 804 << 4 | 32 << 14 | 3 << 22 | 1 << 25) == ("resblock", "fp32", 804, 32, 3, False, True)


def test_tables_partition_what_the_launchers_can_name():
    assert not REACHABLE & UNREACHABLE and REACHABLE | UNREACHABLE == F.compiled()
    assert len(F.compiled()) == 72 + 81 and len(REACHABLE) == 103


def test_reachable_instantiations_are_pinned(lib):
    """Every config of the GPU sweeps x storage type x resblock knob (each of 50..100 too) x LDS limit 0..150: the union of what the
    engine's walk launches is REACHABLE, entry for entry - a change of either picker that moves an instantiation between the two
    tables fails here, before anything runs on a device.  The resblock knob decides which convs exist, the LDS limit their tiles."""
    reached, tiles = set(), {}
    for name, (cfg, *_) in F.CONFIGS.items():
        for precision in F.DTYPES:
            convs = set()
            for knob in ALL_KNOBS:
                with F.knobs(knob, 0):
                    walk = F.layers(lib, cfg, precision, knob)
                convs |= {l[1:7] for l in walk if l[0] == "conv"}
                reached |= {F.instantiation(l) for l in walk if l[0] == "resblock"}
            for limit in range(0, 151):
                with F.knobs(1, limit):
                    for shape in convs:
                        if (precision, limit, shape) not in tiles:
                            tiles[precision, limit, shape] = F.conv_tile(lib, precision, *shape)
                        reached.add(("conv", precision) + tiles[precision, limit, shape])
    assert reached - REACHABLE == set(), sorted(reached - REACHABLE)
    assert REACHABLE - reached == set(), sorted(REACHABLE - reached)


def test_the_sweep_of_the_gpu_tests_reaches_the_whole_table():
    """knob in KNOBS x limit in LIMITS - the cells tests/test_gpu_hifigan_forms.py chooses from - lose nothing against 0..150 / 50..100"""
    got = set()
    for name, (cfg, *_) in F.CONFIGS.items():
        for precision in F.DTYPES:
            for knob in F.KNOBS:
                for limit in F.LIMITS:
                    got |= {F.instantiation(l) for l in F.plan(cfg, precision, knob, limit)}
    assert got == REACHABLE


def test_long_dilation_pair_takes_the_half_height_form(lib):
    """the one geometry with 16-bit 804: 128 channels, k = 11, dilation 9 (and the default heuristic sends a 1024-channel 16-bit
    generator's first upsampler to <T, 2, 0>, the issue's never-executed default path)"""
    cfg = F.CONFIGS["long_dilation"][0]
    for precision in ("bf16", "fp16"):
        assert ("resblock", precision, 804, 128, 1, False, True) in F.plan(cfg, precision, 1, 0)
        assert ("conv", precision, 2, 0, False, False, True) in F.plan(F.CONFIGS["wide"][0], precision, 1, 0)
