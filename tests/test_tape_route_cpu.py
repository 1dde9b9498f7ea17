"""Which training shapes reach the fused tape launches is host arithmetic too (route_gemm through fs2_op_gemm_route): pinned
here without a GPU, as the premise of the GPU tests that are meant to run them.

tests/test_gpu_training.py has two families of small cases: `_case` (hidden 64, filters 96 .. 160), whose GEMMs the slab kernel
does not take in auto mode - the step then runs its GEMM + dropout + LayerNorm fallback - and `_case(..., **WIDE)` (hidden 192,
conv filters 256), where fs2_op_gemm_ln_tape[_dropout], fs2_op_gemm_relu_dropout and fs2_op_gemm_gated all launch.  If routing ever
changes so that a WIDE request below is refused, the WIDE cases of test_gpu_training.py (oracle, derivative under dropout, the
switch comparison) have gone back to testing the fallback only, and tests/test_gpu_tape_ops.py is what is left of the fused
epilogue's coverage."""
import pytest

from lightningfastspeech2_amd import _lib
from test_gemm_route_cpu import PRESENT, decode, lib, set_knobs  # noqa: F401  (lib: the module-scoped fixture that builds on demand)

F32, BF16 = _lib.FS2_F32, _lib.FS2_BF16
ERR_SHAPE = {"status": _lib.FS2_ERR_SHAPE}
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
B = 3
PADDED = [17, 26, 32]  # padded phone / frame counts of the WIDE cases: _case(41, 3, 17, ...) has L = 17, T = 32; _case(31, 3, 12, ...) T = 26


def bits(*names):
    return sum(1 << PRESENT.index(n) for n in names)


def route(lib, dtype, M, N, Cin, taps, S, *present):
    return decode(lib.fs2_op_gemm_route(dtype, dtype, M, N, Cin, taps, S, 0, bits(*present), 1))


TAPE = ("bias", "res", "ln_g", "z_out")
PRED = ("bias", "ln_g", "z_out", "relu")


def fused(a):
    return a.get("family") == "slab" and "LN" in a["flags"] and a["two_launch"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", PADDED)
def test_wide_shapes_take_the_fused_launches(lib, dtype, S):
    """WIDE: hidden 192, conv filters 256, variance / duration filters 192, kernel sizes 5 / 9 / 3 / 5, B = 3."""
    M = B * S
    for drop in ((), ("drop",)):
        assert fused(route(lib, dtype, M, 192, 192, 1, M, *TAPE, *drop)), ("out-proj", drop)
        assert fused(route(lib, dtype, M, 192, 256, 1, M, *TAPE, *drop)), ("conv2", drop)
    for taps in (3, 5):
        assert fused(route(lib, dtype, M, 192, 192, taps, S, *PRED)), ("predictor", taps)
    for taps in (5, 9):  # encoder / decoder conv1
        a = route(lib, dtype, M, 256, 192, taps, S, "bias", "relu", "drop")
        assert a.get("family") == "slab" and "LN" not in a["flags"], ("conv1", taps, a)
    a = route(lib, dtype, M, 256, 192, 1, M, "gate")
    assert a.get("family") == "slab" and "LN" not in a["flags"], ("gate", a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_case_of_twelve_phones_fuses_its_plain_gemms_only(lib, dtype):
    """_case(31, 3, 12, ..., **WIDE) (the derivative test) has L = 12: three 32-row tiles would cover 96 rows for 36, so the
    encoder's conv1 and the duration predictor's convs fall back there; the out-projection and conv2 (one segment of 36 rows) and
    the whole frame side (T = 26, above) still fuse."""
    S, M = 12, 36
    for drop in ((), ("drop",)):
        assert fused(route(lib, dtype, M, 192, 192, 1, M, *TAPE, *drop))
        assert fused(route(lib, dtype, M, 192, 256, 1, M, *TAPE, *drop))
    assert route(lib, dtype, M, 192, 192, 3, S, *PRED) == ERR_SHAPE
    assert route(lib, dtype, M, 256, 192, 5, S, "bias", "relu", "drop") == ERR_SHAPE
    assert route(lib, dtype, M, 256, 192, 1, M, "gate").get("family") == "slab"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [12, 13, 17, 32, 37])
def test_hidden_64_shapes_do_not(lib, dtype, S):
    """`_case` without WIDE: hidden 64, decoder filter 160.  Every fused request is refused, so those tests run the fallback."""
    M = B * S
    for drop in ((), ("drop",)):
        assert route(lib, dtype, M, 64, 64, 1, M, *TAPE, *drop) == ERR_SHAPE
        assert route(lib, dtype, M, 64, 160, 1, M, *TAPE, *drop) == ERR_SHAPE
    for taps in (3, 5):
        assert route(lib, dtype, M, 64, 64, taps, S, *PRED) == ERR_SHAPE
    for taps in (5, 9, 3):
        assert route(lib, dtype, M, 160, 64, taps, S, "bias", "relu", "drop") == ERR_SHAPE
    assert route(lib, dtype, M, 160, 64, 1, M, "gate") == ERR_SHAPE


@pytest.mark.parametrize("dtype", DTYPES)
def test_what_the_tape_launch_refuses(lib, dtype):
    for drop in ((), ("drop",)):
        assert route(lib, dtype, 96, 260, 256, 1, 96, *TAPE, *drop) == ERR_SHAPE         # wider than one column tile
        assert route(lib, dtype, 96, 256, 256, 2, 32, *TAPE, *drop) == ERR_SHAPE         # even tap count
        assert route(lib, dtype, 25, 256, 256, 3, 5, *TAPE, *drop) == ERR_SHAPE          # B = 5, S = 5: 160 tile rows for 25
        assert fused(route(lib, dtype, 96, 256, 256, 3, 32, *TAPE, *drop))               # (the same request where it applies)
        try:
            set_knobs(lib, [1])
            assert route(lib, dtype, 96, 256, 256, 3, 32, *TAPE, *drop) == ERR_SHAPE     # the 128 x 128 kernel forced
        finally:
            set_knobs(lib, [0])
