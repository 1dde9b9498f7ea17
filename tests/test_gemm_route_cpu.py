"""Which kernel serves a GEMM / conv request is host arithmetic (route_gemm, gemm_mfma.hip): pinned here without a GPU.

tests/golden/gemm_route.json holds requests and the answers fs2_op_gemm_route must give.  The answers were NOT produced by route_gemm:
they were recorded from the launcher it replaced (launch_gemm / launch_gemm_plain / launch_slab_do / launch_slab), whose terminal
launch functions were made to write down the kernel instantiation and grid instead of launching, driven with dummy aligned pointers.
So a row says what that code launched (or which status it returned) for the request, and route_gemm has to agree.

One input of the route is the device's: the persistent kernel is chosen where a launch has more tiles than the device has CUs
(256 on the MI355X, and the value assumed where there is no device), so the rows hold for 256 CUs."""
import json
import os

import pytest

from lightningfastspeech2_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_route.json")
F32, BF16, F16 = _lib.FS2_F32, _lib.FS2_BF16, _lib.FS2_F16
FAMILIES = {0: "none", 1: "flat128", 2: "slab", 3: "persist", 4: "wres"}
PRESENT = ["bias", "res", "ln_g", "dot_w", "z_out", "ln_tmp", "stats_out", "epi_res", "gate", "drop", "rs", "head", "zero_rows", "C_lo", "split",
           "w_presplit", "relu"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def decode(v):
    if v < 0:
        return {"status": -v}
    flags = [n for i, n in enumerate(["LN", "SPLIT", "DEFER", "XPRE", "ZR", "presplit"]) if v >> (8 + i) & 1]
    return {"family": FAMILIES[v & 15], "mi": v >> 4 & 15, "flags": flags, "two_launch": v >> 16 & 1}


def describe(row):
    knobs, dt, odt, M, N, Cin, taps, S, ksplit, present, aligned, _ = row
    return dict(knobs=knobs, dtype=dt, out_dtype=odt, M=M, N=N, Cin=Cin, taps=taps, S=S, ksplit=ksplit,
                present=[n for i, n in enumerate(PRESENT) if present >> i & 1], bias_aligned=aligned)


def set_knobs(lib, knobs):
    for k in knobs:
        assert lib.fs2_op_set_gemm_variant(k) == 0, k


def test_route_answers_what_the_replaced_launcher_launched(lib, golden):
    wrong = []
    try:
        for row in golden["rows"]:
            set_knobs(lib, golden["default_knobs"] + row[0])
            got = lib.fs2_op_gemm_route(*row[1:11])
            if got != row[11]:
                wrong.append((describe(row), "expected", decode(row[11]), "got", decode(got)))
    finally:
        set_knobs(lib, golden["default_knobs"])
    assert not wrong, (len(wrong), wrong[:5])


def test_fixture_covers_the_launcher(golden):
    """every forced variant but the retired 2, the knobs the router reads, all nine storage dtype pairs, N on both sides of 192 and
    256, tap counts, S dividing M or not, K on both sides of 4096, every family and every slab flag"""
    rows = golden["rows"]
    assert len(rows) >= 300
    knobs = {k for r in rows for k in r[0]}
    assert {1, 3, 4, 5, 6, 7, 220, 221, 1400, 1401, 1402, 230, 231, 500, 501} <= knobs and 2 not in knobs
    assert {(i, o) for i in (F32, BF16, F16) for o in (F32, BF16, F16)} <= {(r[1], r[2]) for r in rows}
    assert {128, 188, 192, 252, 256, 260} <= {r[4] for r in rows}
    assert {1, 2, 3, 9} <= {r[6] for r in rows}
    assert any(r[3] % r[7] for r in rows if r[7]) and any(r[3] % r[7] == 0 for r in rows if r[7])
    assert any(r[5] * r[6] < 4096 for r in rows) and any(r[5] * r[6] > 4096 for r in rows)
    for bit in range(len(PRESENT)):  # each member alone, and with each other one
        assert any(r[9] == 1 << bit for r in rows), PRESENT[bit]
        for other in range(bit):
            assert any(r[9] == (1 << bit | 1 << other) for r in rows), (PRESENT[bit], PRESENT[other])
    answers = [decode(r[11]) for r in rows]
    assert {a["status"] for a in answers if "status" in a} == {2, 3}  # FS2_ERR_SHAPE and FS2_ERR_ARG
    assert set(FAMILIES.values()) <= {a["family"] for a in answers if "family" in a}
    assert {1, 2, 4, 6, 8} <= {a["mi"] for a in answers if a.get("family") == "slab"}
    assert {"LN", "SPLIT", "DEFER", "XPRE", "ZR", "presplit"} <= {f for a in answers for f in a.get("flags", [])}
    assert any(a.get("two_launch") for a in answers)


def test_retired_ring_variant_is_not_a_route(lib):
    request = (BF16, BF16, 512, 256, 256, 1, 512, 0, 1, 1)
    before = lib.fs2_op_gemm_route(*request)
    assert decode(before)["family"] == "slab"
    assert lib.fs2_op_set_gemm_variant(2) != 0
    assert lib.fs2_op_gemm_route(*request) == before  # still the automatic choice
