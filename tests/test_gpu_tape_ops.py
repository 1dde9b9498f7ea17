"""GPU: the fused launches of the training tape one by one through the C ABI, each against a plain float64 torch reference of
the same operation on the inputs as the kernel sees them (G.rounded):

  fs2_op_gemm_ln_tape / fs2_op_gemm_ln_tape_dropout   GEMM or conv -> ReLU -> dropout -> residual -> LayerNorm + the pre-norm store
  fs2_op_layernorm_bwd_masked                         LayerNorm backward with the residual-site dropout backward as a second tensor
  fs2_op_layernorm_head, fs2_op_row_dot               the predictor heads of the training path

The training step takes these only at widths the slab kernel runs (tests/test_tape_route_cpu.py pins which); a dropout mask is
checked against fs2_op_dropout's for the same (p, seed, key), which is what the backward regenerates.  Bounds are the ones
tests/test_gpu_ops.py and tests/test_gpu_backward_ops.py use for the same kind of comparison.  Each test prints the figure it
asserts on (pytest -s shows it).  Measured on the MI355X, worst case as a share of its bound: tape z 7 % (fp32) / 23 % (bf16),
y 2 % / 14 %; with dropout z 4 % / 30 %, y 2 % / 13 %; no entry off the mask; dz against autograd 0.8 %; every dzm entry bit-equal;
third partial sum 0.3 %; row_dot 3 %."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _gpu as G
from lightningfastspeech2_amd import _lib
from test_gpu_ops import DTYPES, rnd, tol

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_SHAPE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_SHAPE
SEED, KEY, PDROP = 1234567, 7, 0.25

# (B, S, Cin, N, taps, relu, res)
FULL_RAGGED = (3, 37, 256, 256, 1, False, True)     # ragged last 32-row tile, the full-width branch
PREDICTOR = (3, 37, 256, 200, 3, True, False)       # columns past N zeroed (!full), the predictor layer's form
SCALAR_TAIL = (3, 37, 256, 196, 1, False, True)     # last 8-channel group half valid; bf16 rows only 8-byte aligned
RES_AFTER_RELU = (2, 70, 128, 192, 5, True, True)   # residual behind a ReLU: not ridden in the accumulators
LONG_K = (2, 17, 1024, 256, 1, False, True)
LONG_CONV = (1, 300, 256, 256, 9, False, False)
CASES = [FULL_RAGGED, PREDICTOR, SCALAR_TAIL, RES_AFTER_RELU, LONG_K, LONG_CONV]
KNOBS = [pytest.param(0, id="auto"), pytest.param(3, id="slab128"), pytest.param(4, id="slab192"), pytest.param(6, id="slab32"),
         pytest.param(7, id="slab64")]


def _id(case):
    return "B{}_S{}_Cin{}_N{}_k{}{}{}".format(*case[:5], "_relu" if case[5] else "", "_res" if case[6] else "")


@pytest.fixture
def knob(request):
    G.lib().fs2_op_set_gemm_variant(request.param)
    yield request.param
    G.lib().fs2_op_set_gemm_variant(0)


@functools.lru_cache(maxsize=None)
def _tape_case(case, dtype):
    """inputs (fp32, as handed to the helpers) and the float64 pre-activation a = conv_same(x, w) + b per utterance, (M, N)"""
    B, S, Cin, N, k, _, _ = case
    x = rnd(B, S, Cin, seed=50)
    w = rnd(N, Cin, k, seed=51, scale=(Cin * k) ** -0.5)
    b, res = rnd(N, seed=52), rnd(B * S, N, seed=53)
    g, be = 1 + 0.2 * rnd(N, seed=54), 0.1 * rnd(N, seed=55)
    a = F.conv1d(G.rounded(x, dtype).double().transpose(1, 2), G.rounded(w, dtype).double(), b.double(), padding="same")
    a = a.transpose(1, 2).reshape(B * S, N)
    return dict(x=x.reshape(B * S, Cin), w=G.pack_conv_weight(w), b=b, res=res, g=g, be=be, a=a, r64=G.rounded(res, dtype).double())


def _ref(c, relu, res, keep=None):
    """z = [keep o] act(a) [+ res], y = LayerNorm(z), float64"""
    z = torch.relu(c["a"]) if relu else c["a"]
    if keep is not None:
        z = z * keep.double()
    if res:
        z = z + c["r64"]
    return z, F.layer_norm(z, (z.shape[1],), c["g"].double(), c["be"].double(), 1e-5)


def _run(dtype, c, case, relu, res, drop=None, **kw):
    B, S, _, _, k, _, _ = case
    S = S if k > 1 else B * S  # a plain GEMM goes in as one segment, as the training step hands it over
    return G.gemm_ln_tape(dtype, c["x"], c["w"], c["b"], c["res"] if res else None, c["g"], c["be"], k, S, relu, drop=drop, **kw)


def _close(got_buf, ref, bound, what):
    assert G.guard_intact(got_buf), what
    got = got_buf[:-1].double().cpu()
    assert bool(torch.isfinite(got).all()), what  # a row the kernel never wrote still holds the sentinel
    err = float((got - ref).abs().max())
    print(f"{what}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _is_fused(dtype, case, drop):
    B, S, Cin, N, k, relu, res = case
    present = 1 | (2 if res else 0) | 4 | 16 | (512 if drop else 0) | (1 << 16 if relu else 0)  # bias, res, ln_g, z_out, drop, relu
    v = G.lib().fs2_op_gemm_route(dtype, dtype, B * S, N, Cin, k, S if k > 1 else B * S, 0, present, 1)
    return v > 0 and v & 15 == 2 and v >> 8 & 1 and not v >> 16 & 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knob", KNOBS, indirect=True)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gemm_ln_tape(dtype, knob, case):
    """z = act(conv_same(x, w) + b) [+ res] per utterance and y = LayerNorm(z), both stored by one launch; y is bit for bit what
    fs2_op_gemm_ln gives on the same inputs and knob (the pre-norm store is a side output, not another arithmetic)."""
    B, S, _, _, k, relu, res = case
    c = _tape_case(case, dtype)
    assert _is_fused(dtype, case, False)
    zr, yr = _ref(c, relu, res)
    st, y, z = _run(dtype, c, case, relu, res)
    G.ok(st, "gemm_ln_tape")
    _close(z, zr, tol(dtype, zr), "z")
    _close(y, yr, tol(dtype, yr, f32=5e-5, bf16=2.5e-2), "y")
    plain, _ = G.gemm_ln(dtype, c["x"], c["w"], c["b"], c["res"] if res else None, c["g"], c["be"], taps=k, S=S if k > 1 else B * S, relu=relu, raw=True)
    assert torch.equal(G.bits(y[:-1]), G.bits(plain))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knob", [pytest.param(0, id="auto"), pytest.param(3, id="slab128"), pytest.param(6, id="slab32")], indirect=True)
@pytest.mark.parametrize("case", [FULL_RAGGED, SCALAR_TAIL, RES_AFTER_RELU], ids=_id)
def test_gemm_ln_tape_dropout_mask_is_the_dropout_ops(dtype, knob, case):
    """Without residual and ReLU the stored z is zero exactly where the element was dropped: the pattern must be fs2_op_dropout's
    for the same (p, seed, key) over the (M, N) element index - several utterances of a conv (row base = utterance x S), N < 256
    (the index runs over N, not the tile width) and a ragged last row tile."""
    B, S, _, N, _, _, _ = case
    c = _tape_case(case, dtype)
    assert _is_fused(dtype, case[:5] + (False, False), True)
    assert float(c["a"].abs().min()) > 0  # no product entry is itself 0 (nor anywhere near a 16-bit underflow)
    keep = G.dropout_keep((B * S, N), PDROP, SEED, KEY)
    st, y, z = _run(dtype, c, case, False, False, drop=(PDROP, SEED, KEY))
    G.ok(st, "gemm_ln_tape_dropout")
    assert G.guard_intact(y) and G.guard_intact(z)
    got = z[:-1].float().cpu()
    assert bool(torch.isfinite(got).all())
    share = float((keep == 0).float().mean())
    wrong = int(((got == 0) != (keep == 0)).sum())
    print(f"dropped share {share:.4f}, entries off the mask {wrong}")
    assert 0.2 < share < 0.3
    assert wrong == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knob", [pytest.param(0, id="auto"), pytest.param(3, id="slab128")], indirect=True)
@pytest.mark.parametrize("case", [FULL_RAGGED, PREDICTOR, RES_AFTER_RELU], ids=_id)
def test_gemm_ln_tape_dropout_values(dtype, knob, case):
    """z = keep o act(.) / (1 - p) + res (the dropout sits between the activation and the residual add), y = LayerNorm(z)."""
    B, S, _, N, _, relu, res = case
    c = _tape_case(case, dtype)
    assert _is_fused(dtype, case, True)
    keep = G.dropout_keep((B * S, N), PDROP, SEED, KEY)  # 0 or 1 / (1 - p)
    zr, yr = _ref(c, relu, res, keep)
    st, y, z = _run(dtype, c, case, relu, res, drop=(PDROP, SEED, KEY))
    G.ok(st, "gemm_ln_tape_dropout")
    _close(z, zr, tol(dtype, zr), "z")
    _close(y, yr, tol(dtype, yr, f32=5e-5, bf16=2.5e-2), "y")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [SCALAR_TAIL, RES_AFTER_RELU], ids=_id)
def test_gemm_ln_tape_dropout_with_p_zero_is_the_plain_tape_launch(dtype, case):
    _, _, _, _, _, relu, res = case
    c = _tape_case(case, dtype)
    st0, y0, z0 = _run(dtype, c, case, relu, res)
    st1, y1, z1 = _run(dtype, c, case, relu, res, drop=(0.0, SEED, KEY))
    G.ok(st0, "gemm_ln_tape")
    G.ok(st1, "gemm_ln_tape_dropout")
    assert torch.equal(G.bits(y0), G.bits(y1)) and torch.equal(G.bits(z0), G.bits(z1))  # (guard rows included)


@pytest.mark.parametrize("drop", [None, (PDROP, SEED, KEY)], ids=["tape", "tape_dropout"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_ln_tape_refusals_write_nothing(dtype, drop):
    B, S, Cin, N = 3, 37, 256, 256
    M = B * S
    x, res = rnd(M, Cin, seed=1), rnd(M, N, seed=2)

    def call(N=N, taps=1, S=M, dt=dtype, drop=drop, want_z=True):
        w = rnd(N, taps * Cin, seed=3, scale=(taps * Cin) ** -0.5)
        st, y, z = G.gemm_ln_tape(dt, x, w, rnd(N, seed=4), res[:, :1].expand(M, N), torch.ones(N), torch.zeros(N), taps, S, False,
                                  drop=drop, want_z=want_z)
        assert G.untouched(y) and (z is None or G.untouched(z)), (N, taps, S, dt, drop, want_z)
        return st

    st, y, z = G.gemm_ln_tape(dtype, x, rnd(N, Cin, seed=3), rnd(N, seed=4), res, torch.ones(N), torch.zeros(N), 1, M, False, drop=drop)
    assert st == 0 and not G.untouched(y) and not G.untouched(z)  # the request the refused ones differ from by one thing each
    assert call(want_z=False) == ERR_ARG
    assert call(dt=G.F16) == ERR_ARG
    assert call(N=260) == ERR_SHAPE
    assert call(taps=2, S=S) == ERR_SHAPE
    G.lib().fs2_op_set_gemm_variant(1)
    try:
        assert call() == ERR_SHAPE
    finally:
        G.lib().fs2_op_set_gemm_variant(0)
    if drop is not None:
        assert call(drop=(1.0, SEED, KEY)) == ERR_ARG


# ---- fs2_op_layernorm_bwd_masked -------------------------------------------------------------------------------------------------
OUT_P = 0.3


@functools.lru_cache(maxsize=None)
def _lnb_case(M, H, dtype):
    z, r, dy = (G.rounded(rnd(M, H, seed=60 + i), dtype) for i in range(3))
    return z, r, dy, 1 + 0.3 * rnd(H, seed=63)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu_mask", [0, 1])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("M,H", [(1, 48), (33, 256), (257, 300), (64, 768), (40, 1024)])
def test_layernorm_bwd_masked(dtype, M, H, res, relu_mask):
    """y = LayerNorm(res + dropout(u)): dz and the dgamma / dbeta partial sums are fs2_op_layernorm_bwd's bit for bit; the second
    tensor is dzm = keep ? store(dz_stored * 1 / (1 - p)) : 0 with fs2_op_dropout's mask for (p, seed, key) and the factor in fp32 -
    bit equality holds: the product of the stored dz with the fp32 factor is rounded once on both sides - and the third
    partial sum is the column sum of the stored dzm.  (With a residual AND relu_mask the kernel tests the sum z + res, which is
    what the tape hands over as z when the forward stored the sum.)"""
    z, r, dy, gam = _lnb_case(M, H, dtype)
    r = r if res else None
    st0, dz0, _, part0 = G.layernorm_bwd_s(dtype, z, r, dy, gam, relu_mask)
    st, dz, dzm, part = G.layernorm_bwd_s(dtype, z, r, dy, gam, relu_mask, masked=(OUT_P, SEED, KEY))
    G.ok(st0, "layernorm_bwd")
    G.ok(st, "layernorm_bwd_masked")
    assert all(G.guard_intact(t) for t in (dz0, part0, dz, dzm, part))
    assert bool(torch.isfinite(dz[:-1]).all()) and bool(torch.isfinite(dzm[:-1]).all()) and bool(torch.isfinite(part[:-1]).all())
    assert torch.equal(G.bits(dz), G.bits(dz0))
    nparts = G.lib().fs2_op_layernorm_bwd_parts(M)
    p3, p30 = part[:-1].reshape(nparts, 3, H).cpu(), part0[:-1].reshape(nparts, 3, H).cpu()
    assert torch.equal(G.bits(p3[:, :2]), G.bits(p30[:, :2]))
    if dtype == G.F32:
        zz = (z.double() + (r.double() if res else 0)).requires_grad_(True)
        F.layer_norm(zz, (H,), gam.double(), torch.zeros(H, dtype=torch.float64), 1e-5).backward(dy.double())
        want = torch.where(zz.detach() > 0, zz.grad, torch.zeros((), dtype=torch.float64)) if relu_mask else zz.grad
        err, scale = float((dz[:-1].double().cpu() - want).abs().max()), float(want.abs().max()) + 1e-30
        print(f"dz vs autograd: err {err:.3e} bound {2e-5 * scale:.3e}")
        assert err <= 2e-5 * scale
    keep = G.dropout_keep((M, H), OUT_P, SEED, KEY) != 0
    share = float((~keep).float().mean())
    assert M * H < 4096 or 0.25 < share < 0.35
    sc = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(OUT_P, dtype=torch.float32))
    stored = dz[:-1].cpu()
    want_m = torch.where(keep, (stored.float() * sc).to(stored.dtype), torch.zeros((), dtype=stored.dtype))
    off = int((G.bits(dzm[:-1]) != G.bits(want_m)).sum())
    print(f"dzm entries that are not the masked, scaled dz bit for bit: {off}")
    assert off == 0
    col = dzm[:-1].double().cpu().sum(0)
    err, scale = float((p3[:, 2].double().sum(0) - col).abs().max()), float(col.abs().max()) + 1e-30
    print(f"third partial sum vs column sums of dzm: err {err:.3e} bound {5e-5 * scale:.3e}")
    assert err <= 5e-5 * scale


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bwd_masked_refusals_write_nothing(dtype):
    z, r, dy, gam = _lnb_case(33, 256, dtype)
    for kw in (dict(masked=(OUT_P, SEED, KEY), want_dzm=False), dict(masked=(0.0, SEED, KEY)), dict(masked=(1.0, SEED, KEY))):
        st, dz, dzm, part = G.layernorm_bwd_s(dtype, z, r, dy, gam, 0, **kw)
        assert st == ERR_ARG, kw
        assert G.untouched(dz) and G.untouched(part) and (dzm is None or G.untouched(dzm)), kw


# ---- fs2_op_layernorm_head, fs2_op_row_dot ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,H", [(5, 64), (130, 256), (9, 768)])
def test_layernorm_head_reads_the_bias_from_the_device(dtype, M, H):
    """The same launch as fs2_op_layernorm with its fused head, the head's bias a device scalar: y and pred bit for bit."""
    x, r = rnd(M, H, seed=13, scale=2.0), rnd(M, H, seed=14)
    g, b = 1 + 0.2 * rnd(H, seed=15), 0.1 * rnd(H, seed=16)
    w = rnd(H, seed=17, scale=H ** -0.5)
    mask = torch.zeros(M, dtype=torch.bool)
    mask[::3] = True
    want_y, want_p = G.layernorm(dtype, x, r, g, b, dot_w=w, dot_b=0.3, mask=mask, raw=True)
    st, y, pred = G.layernorm_head_s(dtype, x, r, g, b, w, 0.3, mask)
    G.ok(st, "layernorm_head")
    assert G.guard_intact(y) and G.guard_intact(pred)
    assert torch.equal(G.bits(y[:-1]), G.bits(want_y))
    assert torch.equal(G.bits(pred[:-1, 0]), G.bits(want_p))
    assert bool((pred[:-1, 0].cpu()[mask] == 0).all()) and bool((pred[:-1, 0].cpu()[~mask] != 0).all())
    for kw in (dict(dtype=G.F16), dict(dot_w=None), dict(dot_b=None), dict(want_pred=False)):
        a = dict(dtype=dtype, dot_w=w, dot_b=0.3, want_pred=True)
        a.update(kw)
        st, y, pred = G.layernorm_head_s(a["dtype"], x, r, g, b, a["dot_w"], a["dot_b"], mask, want_pred=a["want_pred"])
        assert st == ERR_ARG, kw
        assert G.untouched(y) and (pred is None or G.untouched(pred)), kw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("H", [48, 64, 200, 1024])
@pytest.mark.parametrize("M", [1, 5, 130])
def test_row_dot(dtype, M, H, masked):
    """pred[m] = mask[m] ? 0 : y[m] . w + b[0]: one wave per row, four rows per workgroup (M = 1, 5, 130 end in a partial one),
    H below a wave's 64 lanes and no multiple of them."""
    y, w = rnd(M, H, seed=70), rnd(H, seed=71, scale=H ** -0.5)
    mask = None
    if masked:
        mask = torch.zeros(M, dtype=torch.bool)
        mask[::2] = True
    ref = G.rounded(y, dtype).double() @ w.double() + float(torch.tensor(0.3, dtype=torch.float32))
    if masked:
        ref = ref.masked_fill(mask, 0)
    st, pred = G.row_dot_s(dtype, y, w, 0.3, mask)
    G.ok(st, "row_dot")
    assert G.guard_intact(pred)
    got = pred[:-1, 0].double().cpu()
    assert bool(torch.isfinite(got).all())
    err, scale = float((got - ref).abs().max()), float(ref.abs().max()) + 1e-30
    print(f"row_dot: err {err:.3e} bound {1e-5 * scale:.3e}")
    assert err <= 1e-5 * scale
    if masked:
        assert bool((got[mask] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_dot_refuses_an_empty_batch(dtype):
    st, pred = G.row_dot_s(dtype, torch.zeros(0, 64), rnd(64, seed=1), 0.3, None)
    assert st == ERR_SHAPE and G.untouched(pred)
