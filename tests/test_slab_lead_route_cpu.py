"""Which K loop the slab kernel runs for a request is host arithmetic (slab_lead_form in gemm_mfma.hip, asked through
fs2_op_gemm_route_lead): pinned here without a GPU - where the lead-2 loop EXISTS (knob 242), that knob 240 takes it nowhere, and the
launch classes the default (241) routes to it: exactly the three that measured faster (profiles/slab_lead_ab.md)."""
import os

import pytest

from lightningfastspeech2_amd import _lib

F32, BF16, F16 = _lib.FS2_F32, _lib.FS2_BF16, _lib.FS2_F16
BIAS, RES, LN, LNTMP, STATS, EPIRES, RELU = 1 << 0, 1 << 1, 1 << 2, 1 << 5, 1 << 6, 1 << 7, 1 << 16
LNRES = BIAS | RES | LN | LNTMP
HEIGHTS = {6: 1, 7: 2, 3: 4, 4: 6}  # forced-height knob -> tile rows / 32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def default_knobs(lib):
    yield
    assert lib.fs2_op_set_gemm_variant(241) == 0 and lib.fs2_op_set_gemm_variant(0) == 0


def lead(lib, M, N, Cin, taps, S, present, dtype=BF16, out_dtype=None):
    return lib.fs2_op_gemm_route_lead(dtype, dtype if out_dtype is None else out_dtype, M, N, Cin, taps, S, 0, present, 1)


def route(lib, M, N, Cin, taps, S, present):
    v = lib.fs2_op_gemm_route(BF16, BF16, M, N, Cin, taps, S, 0, present, 1)
    return v & 15, v >> 4 & 15  # family (2 = slab), tile rows / 32


# (M, N, Cin, taps, S, present) -> the form per forced tile height {32, 64, 128, 192 rows}
EXISTS = [
    ((400, 256, 256, 1, 400, BIAS), {1: 1, 2: 1, 4: 1, 6: 1}),             # pointwise, plain epilogue: every height up to 192 rows
    ((400, 256, 64, 1, 400, BIAS | RELU), {1: 1, 2: 1, 4: 1, 6: 1}),       # one K step
    ((400, 256, 1024, 1, 400, LNRES), {1: 1, 2: 1, 4: 1, 6: 0}),           # LayerNorm epilogue: not at 192 rows (spills there: not built)
    ((400, 768, 256, 1, 400, BIAS | STATS | EPIRES), {4: 1, 6: 0}),        # deferred epilogue: likewise
    ((400, 320, 64, 3, 200, BIAS), {1: 2, 2: 2, 4: 2, 6: 0}),              # conv, k = 3 / 9: up to 128 rows (LDS)
    ((400, 256, 256, 9, 200, BIAS | RELU | LN | LNTMP), {1: 2, 2: 2, 4: 2, 6: 0}),
    ((400, 256, 256, 5, 200, BIAS), {1: 0, 2: 0, 4: 0, 6: 0}),             # taps not a multiple of 3: the stage of a step is no static name
    ((400, 256, 256, 7, 200, BIAS), {1: 0, 2: 0, 4: 0, 6: 0}),
]


@pytest.mark.parametrize("req,forms", EXISTS)
def test_where_the_lead2_loop_exists(lib, req, forms):
    for knob, mi in HEIGHTS.items():
        if mi not in forms:
            continue
        assert lib.fs2_op_set_gemm_variant(knob) == 0
        assert route(lib, *req) == (2, mi), (req, knob)
        assert lib.fs2_op_set_gemm_variant(242) == 0
        assert lead(lib, *req) == forms[mi], (req, mi)
        assert lib.fs2_op_set_gemm_variant(240) == 0
        assert lead(lib, *req) == 0, (req, mi)
        if mi == 4:  # 16-bit operands stored as they came in only
            assert lib.fs2_op_set_gemm_variant(242) == 0
            assert lead(lib, *req, dtype=F16) == forms[mi]
            assert lead(lib, *req, dtype=F32) == 0
            if not req[5] & (LN | STATS):
                assert lead(lib, *req, dtype=BF16, out_dtype=F32) == 0


def test_256_row_tiles_and_other_families_have_none(lib):
    assert lib.fs2_op_set_gemm_variant(242) == 0
    assert lib.fs2_op_set_gemm_variant(5) == 0
    assert route(lib, 49152, 1024, 256, 9, 1536, BIAS | RELU) == (2, 8) and lead(lib, 49152, 1024, 256, 9, 1536, BIAS | RELU) == 0
    assert lib.fs2_op_set_gemm_variant(1) == 0
    assert lead(lib, 400, 256, 256, 1, 400, BIAS) == 0
    assert lib.fs2_op_set_gemm_variant(0) == 0
    assert route(lib, 49152, 768, 256, 1, 49152, BIAS)[0] == 4 and lead(lib, 49152, 768, 256, 1, 49152, BIAS) == 0  # weight-resident kernel


# the C2 forward's launches (B = 32, L = 256, T = 1536) and their neighbours under the DEFAULT switches: (request, tile rows / 32, form)
DEFAULT = [
    ((8192, 1024, 256, 9, 256, BIAS | RELU), 4, 2),       # encoder conv1: routed
    ((8192, 256, 1024, 1, 8192, LNRES), 1, 1),            # encoder conv2 + residual + LayerNorm: routed
    ((8192, 256, 256, 3, 256, BIAS | RELU | LN | LNTMP), 1, 2),  # 32-row k = 3 + LayerNorm: routed
    ((8192, 768, 256, 1, 8192, BIAS), 4, 0),              # encoder in-projection (K = 256: at its spread)
    ((8192, 256, 256, 1, 8192, LNRES), 1, 0),             # encoder out-projection + LayerNorm (K = 256)
    ((49152, 256, 1024, 1, 49152, LNRES), 6, 0),          # decoder conv2 + LayerNorm: no form at 192 rows
    ((49152, 256, 256, 1, 49152, LNRES), 6, 0),           # decoder out-projection + LayerNorm
    ((49152, 256, 256, 3, 1536, BIAS | RELU | LN | LNTMP), 6, 0),
    ((49152, 1024, 256, 9, 1536, BIAS | RELU), 8, 0),     # decoder conv1: 256-row tiles
    ((8192, 1024, 256, 3, 256, BIAS | RELU), 4, 0),       # not measured: k = 3 plain at 128 rows
    ((8192, 256, 256, 9, 256, BIAS | RELU | LN | LNTMP), 1, 0),  # not measured: k = 9 + LayerNorm at 32 rows
    ((8192, 256, 2048, 1, 8192, LNRES), 1, 0),            # not measured: K = 2048
    ((8192, 256, 1024, 1, 8192, BIAS), 1, 0),             # not measured: 32-row plain
]


@pytest.mark.parametrize("req,mi,form", DEFAULT)
def test_default_route_takes_the_measured_classes_only(lib, req, mi, form):
    assert lib.fs2_op_set_gemm_variant(241) == 0 and lib.fs2_op_set_gemm_variant(0) == 0
    assert route(lib, *req) == (2, mi), req
    assert lead(lib, *req) == form, req
    assert lib.fs2_op_set_gemm_variant(240) == 0
    assert lead(lib, *req) == 0


def test_the_decision_does_not_look_at_the_batch(lib):
    """the same launch class at another utterance count keeps its form as long as the tile height is the same"""
    assert lib.fs2_op_set_gemm_variant(241) == 0 and lib.fs2_op_set_gemm_variant(0) == 0
    for nb in (32, 16, 64):
        req = (nb * 256, 1024, 256, 9, 256, BIAS | RELU)
        if route(lib, *req) == (2, 4):
            assert lead(lib, *req) == 2, nb
