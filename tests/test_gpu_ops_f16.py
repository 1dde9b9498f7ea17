"""Per-kernel parity of the FS2_F16 operators (`-m gpu`): every operator entry point that takes IEEE binary16 storage, through the C
ABI, against fp32 torch math on the f16-rounded inputs.  The kernels are the bf16 ones instantiated for another 16-bit type: the
assertions have the form of tests/test_gpu_ops.py's bf16 cases with the output's unit roundoff moved by 2^3 - 1.5e-3 (3 * 2^-11 of
the output scale) where bf16 has 1.2e-2 (3 * 2^-8), 3.2e-3 for 2.5e-2 behind a LayerNorm epilogue.  Shapes are the smallest that
reach each code path (partial tiles, more than one workgroup, every kernel family)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import _f16 as H16
import _gpu as G
from lightningfastspeech2_amd import _lib

pytestmark = pytest.mark.gpu

F32, F16 = G.F32, G.F16
T16 = torch.float16
UNIT, UNIT_LN = 1.5e-3, 3.2e-3


def tol(ref, unit=UNIT):
    return unit * (float(ref.abs().max()) + 1e-6)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def r16(x):
    return H16.rnd16(x, T16)


def knob(v):
    assert G.lib().fs2_op_set_gemm_variant(v) == 0


def pack_conv_weight(w):
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


@pytest.fixture(params=[1, 3, 4, 5, 6, 7], ids=["gemm128x128", "slab128", "slab192", "slab256", "slab32", "slab64"])
def gemm_variant(request):
    knob(request.param)
    yield request.param
    knob(0)


# ---- conversion: the saturation rule, bit for bit ------------------------------------------------------------------------------
def test_convert_f32_f16_f32_is_the_host_rule_bit_for_bit():
    """fp32 -> FS2_F16 on the device gives the bits of clamp(+-65504) + round-to-nearest-even on every class of input (normals,
    ties, subnormals, the largest finite value and beyond, infinities -> +-65504, signed zeros, NaN -> NaN); back to fp32 exactly."""
    x = H16.edge_values()
    h = G.convert(F32, F16, x.to(G.DEV))
    assert h.dtype == T16
    got, want = h.cpu().view(torch.int16), H16.f16_bits(x)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, [(float(x[i]), hex(int(got[i]) & 0xFFFF), hex(int(want[i]) & 0xFFFF)) for i in bad[:8]]
    back = G.convert(F16, F32, h).cpu()
    ref = want.view(T16).float()
    nan = torch.isnan(x)
    assert torch.equal(back[~nan], ref[~nan]) and bool(torch.isnan(back[nan]).all())
    assert float(back[~nan].abs().max()) == 65504.0
    same = G.convert(F16, F16, h).cpu().view(torch.int16)
    assert torch.equal(same[~nan], want[~nan])


def test_convert_takes_tensors_and_streams_as_they_are():
    """The binding's converter against explicit pointers on a side stream: (tensor | c_void_p of its data_ptr) x (torch.cuda.Stream |
    c_void_p of its handle) give the same bits, the host rule's.  1027 values: neither whole 256-thread blocks nor whole 16-byte vectors."""
    e = H16.edge_values()
    x = torch.cat([e[::e.numel() // 1000][:1006], e[-21:]]).contiguous()
    assert x.numel() == 1027
    xd = x.to(G.DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    outs = []
    handle = side.cuda_stream
    for explicit in (False, True):
        for st in (side, C.c_void_p(handle)):
            out = torch.full((1027 + 5,), 7.0, dtype=T16, device=G.DEV)
            torch.cuda.synchronize()
            src, dst = xd.data_ptr(), out.data_ptr()
            args = (C.c_void_p(src), C.c_void_p(dst)) if explicit else (xd, out)
            G.ok(G.lib().fs2_op_convert(F32, F16, *args, 1027, st), "convert")
            side.synchronize()
            outs.append(out.cpu())
    want = H16.f16_bits(x)
    for out in outs:
        assert torch.equal(out[:1027].view(torch.int16), want) and bool((out[1027:] == 7.0).all())


# ---- GEMM / conv ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dt", [pytest.param(F16, id="f16out"), pytest.param(F32, id="f32out")])
@pytest.mark.parametrize("M,N,K", [(37, 4, 64), (200, 80, 64), (300, 260, 256), (513, 1024, 1024)])
def test_gemm_plain(M, N, K, out_dt, gemm_variant):
    x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    ref = r16(x) @ r16(w).T + b   # asymmetric, transpose-detecting
    got = G.gemm(F16, x, w, b, out_dtype=out_dt, raw=True)
    assert got.dtype == (T16 if out_dt == F16 else torch.float32)
    err = float((got.float() - ref).abs().max())
    assert err <= tol(ref), (err, tol(ref))


def test_gemm_store_saturates_instead_of_overflowing():
    """A product beyond the binary16 range is stored as +-65504 (finite), not as an infinity; the fp32 store keeps the value."""
    M, N, K = 40, 256, 64
    x, w = torch.full((M, K), 60.0), torch.full((N, K), 30.0)
    w[1::2] = -30.0
    b = torch.zeros(N)
    got = G.gemm(F16, x, w, b).float()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[:, 0::2], torch.full((M, N // 2), 65504.0)) and torch.equal(got[:, 1::2], torch.full((M, N // 2), -65504.0))
    assert torch.equal(G.gemm(F16, x, w, b, relu=True).float()[:, 1::2], torch.zeros(M, N // 2))
    assert float(G.gemm(F16, x, w, b, out_dtype=F32)[0, 0]) == 60.0 * 30.0 * K


@pytest.mark.parametrize("variant", [0, 1, 3], ids=["auto", "gemm128x128", "slab128"])
@pytest.mark.parametrize("B,S,Cin,N,k", [(3, 50, 256, 1024, 9), (2, 33, 768, 768, 1)])
def test_gemm_conv_same_padding_per_utterance(B, S, Cin, N, k, variant):
    x = rnd(B, S, Cin, seed=7)
    w = rnd(N, Cin, k, seed=8, scale=(Cin * k) ** -0.5)
    b = rnd(N, seed=9)
    ref = F.conv1d(r16(x).transpose(1, 2), r16(w), b, padding="same").transpose(1, 2)
    knob(variant)
    try:
        got = G.gemm(F16, x.reshape(B * S, Cin), pack_conv_weight(w), b, taps=k, S=S).float().reshape(B, S, N)
    finally:
        knob(0)
    err = float((got - ref).abs().max())
    assert err <= tol(ref), (err, tol(ref))


@pytest.mark.parametrize("B,S,Cin,N,k,relu", [(2, 77, 256, 256, 3, False), (3, 50, 1024, 256, 1, True), (2, 50, 768, 768, 1, False)])
def test_gemm_residual_layernorm_epilogue(B, S, Cin, N, k, relu):
    """conv / GEMM -> (+ ReLU) -> + residual -> LayerNorm: in the slab kernel's epilogue for one column tile (N = 256), as a GEMM
    launch + the LayerNorm kernel for wider rows (N = 768); twice, same bits.  (The other N = 768 form - deferred statistics +
    rowstats_finish + the row-scaled GEMM - is test_deferred_statistics_then_rowscaled_gemm_is_layernorm_then_gemm.)"""
    x = rnd(B, S, Cin, seed=50)
    w = rnd(N, Cin, k, seed=51, scale=(Cin * k) ** -0.5)
    b, res = rnd(N, seed=52), rnd(B * S, N, seed=53)
    g, be = 1 + 0.2 * rnd(N, seed=54), 0.1 * rnd(N, seed=55)
    z = F.conv1d(r16(x).transpose(1, 2), r16(w), b, padding="same").transpose(1, 2).reshape(B * S, N)
    z = (torch.relu(z) if relu else z) + r16(res)
    ref = F.layer_norm(z, (N,), g, be, 1e-5)
    run = lambda: G.gemm_ln(F16, x.reshape(B * S, Cin), pack_conv_weight(w), b, res, g, be, taps=k, S=S, relu=relu, raw=True)[0]
    y, again = run(), run()
    assert torch.equal(y.view(torch.int16), again.view(torch.int16))
    assert float((y.float() - ref).abs().max()) <= tol(ref, UNIT_LN)


@pytest.mark.parametrize("M,N,K", [(300, 768, 256), (77, 712, 384)])
def test_gemm_with_addend(M, N, K):
    """c = x w^T + bias + addend: the residual-in-the-accumulators path of the deferred epilogue."""
    x, w, b, add = rnd(M, K, seed=31), rnd(N, K, seed=32, scale=K ** -0.5), rnd(N, seed=33), rnd(M, N, seed=34)
    ref = r16(x) @ r16(w).T + b + r16(add)
    got = G.gemm_add(F16, x, w, b, add, in_place=False)
    assert float((got - ref).abs().max()) <= tol(ref)


@pytest.mark.parametrize("M,Kin,K,N,out_dt", [
    (24576, 384, 768, 1024, F16),   # 128 x 3 tiles of 192 rows (deferred epilogue) and 128 x 4 (row-scaled): 1.5 / 2 tiles per workgroup
    (49152, 128, 768, 2304, F16),   # the C3 in-projection: 192 x 9 tiles of 256 rows, 6.75 per workgroup (the 256-row row-scaled form)
    (333, 128, 768, 200, F16),      # ragged row tile, a column tail
    (500, 256, 768, 80, F32)])      # a narrow head behind the folded LayerNorm (the mel Linear): 128x128 kernel, fp32 out
def test_deferred_statistics_then_rowscaled_gemm_is_layernorm_then_gemm(M, Kin, K, N, out_dt):
    """What a wide depth-wise f16 block does between two GEMMs, operator by operator: the deferred-LayerNorm epilogue (GEMM + residual
    -> pre-norm rows v in f16 + per-tile (sum, sum of squares); fs2_op_gemm_stats), fs2_op_rowstats_finish, then the next GEMM on v with
    the norm folded into its operands and (rstd, rstd * mean) applied per row (fs2_op_gemm_rowscale_dt).  Against LayerNorm-then-GEMM in
    fp32 on the stored v; the statistics against the fp32 rows; both launches bit-equal between the one-tile-per-workgroup slab kernel
    (knob 220) and the persistent kernel (221) - gemm_persist_kernel<f16, 6, DEFER> and <f16, 6 | 8, RS> at the first shape -, twice."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(M, Kin, generator=g)
    w1 = torch.randn(K, Kin, generator=g) * 1.7 / math.sqrt(Kin)
    b1 = 0.4 * torch.randn(K, generator=g)
    res = torch.randn(M, K, generator=g) + 0.4 * torch.randn(M, 1, generator=g)   # rows with their own mean
    w0 = torch.randn(N, K, generator=g) / math.sqrt(K)
    b0 = torch.randn(N, generator=g) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    wf = r16(w0 * gamma[None, :])                                       # as stored
    bf = (b0.double() + w0.double() @ beta.double()).float()
    wg = wf.double().sum(1).float()
    runs = {}
    try:
        for kn in (220, 221, 221):
            knob(kn)
            v, st = G.gemm_stats(F16, x, w1, b1, res)
            runs.setdefault(kn, []).append((v.cpu(), st.cpu(), G.gemm_rowscale_dt(F16, v, st, wf, bf, wg, out_dtype=out_dt)))
    finally:
        knob(221)
    (v0, st0, c0), (v1, st1, c1), (v2, st2, c2) = runs[220][0], runs[221][0], runs[221][1]
    for a, b in ((v0, v1), (v1, v2)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(st0, st1) and torch.equal(st1, st2) and bool(torch.isfinite(st1).all())
    assert torch.equal(c0, c1) and torch.equal(c1, c2)
    R = min(M, 2048)   # (rows are independent: the fp32 reference on the first and the last 1024 of them)
    rows = torch.cat([torch.arange(R // 2), torch.arange(M - (R - R // 2), M)])
    x, res, v1, st1, c1 = x[rows], res[rows], v1[rows], st1[rows], c1[rows]
    vref = r16(x) @ r16(w1).T + b1 + r16(res)
    assert float((v1.float() - vref).abs().max()) <= tol(vref)
    s1, s2 = st1[:, :, 0].sum(1), st1[:, :, 1].sum(1)
    assert float((s1 - vref.sum(1)).abs().max()) <= 1e-4 * float(vref.abs().sum(1).max())
    assert float((s2 - (vref * vref).sum(1)).abs().max()) <= 1e-4 * float((vref * vref).sum(1).max())
    ref = F.layer_norm(v1.float(), (K,), gamma, beta, 1e-5) @ w0.T + b0
    err = float((c1.float() - ref).abs().max())
    assert err <= 2.5 * tol(ref), (err, tol(ref))      # f16 W' (2^-12 per weight) + the statistics of the unrounded rows + the f16 output


@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("M", [1, 95, 97, 96 * 9 + 5])
def test_wres_gemm_is_bit_identical_to_the_slab_kernel(M, N):
    x, w, b = rnd(M, 256, seed=3), rnd(N, 256, seed=4) / 16, rnd(N, seed=5)
    try:
        knob(1400)
        old = G.gemm(F16, x, w, b, relu=(N == 256), raw=True)
        knob(1402)   # the weight-resident kernel at every size
        got = G.gemm(F16, x, w, b, relu=(N == 256), raw=True)
        again = G.gemm(F16, x, w, b, relu=(N == 256), raw=True)
    finally:
        knob(1401)
    assert torch.equal(got.view(torch.int16), old.view(torch.int16)) and torch.equal(got.view(torch.int16), again.view(torch.int16))
    ref = r16(x) @ r16(w).T + b
    ref = ref.clamp_min(0) if N == 256 else ref
    assert float((got.float() - ref).abs().max()) <= tol(ref)


@pytest.mark.parametrize("M,N,K,add", [(70001, 512, 128, False),   # 548 tiles of 256 rows on 256 workgroups: 2-3 tiles each, ragged last tile
                                        (50000, 256, 128, True)])   # deferred epilogue (192-row tiles): 261 tiles, a second round for some
def test_persistent_gemm_is_bit_identical_to_the_slab_kernel(M, N, K, add):
    x, w, b = rnd(M, K, seed=31), rnd(N, K, seed=32) / math.sqrt(K), rnd(N, seed=33)
    addend = rnd(M, N, seed=34) if add else None
    run = (lambda: G.gemm_add(F16, x, w, b, addend, in_place=False, raw=True)) if add else (lambda: G.gemm(F16, x, w, b, relu=True, raw=True))
    try:
        knob(220)
        old = run()
        knob(221)
        got, again = run(), run()
    finally:
        knob(221)
    assert torch.equal(got.view(torch.int16), old.view(torch.int16)) and torch.equal(got.view(torch.int16), again.view(torch.int16))
    ref = r16(x) @ r16(w).T + b
    ref = ref + r16(addend) if add else ref.clamp_min(0)
    assert float((got.float() - ref).abs().max()) <= tol(ref)


# ---- attention -----------------------------------------------------------------------------------------------------------------
def _attn_ref(qkv, mask, B, S, H, heads):
    d = H // heads
    q, k, v = qkv.view(B, S, 3 * H).split(H, dim=-1)
    q = q.view(B, S, heads, d).transpose(1, 2) * (1.0 / math.sqrt(d))
    k = k.view(B, S, heads, d).transpose(1, 2)
    v = v.view(B, S, heads, d).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)).masked_fill(mask[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * S, H)


def _mask(kind, B, S):
    mask = torch.zeros(B, S, dtype=torch.bool)
    if kind == "ragged":
        for b in range(B):
            mask[b, S - (7 + 13 * b) % S:] = True
        mask[0, :] = False
        mask[0, S - S // 2:] = True
    elif kind == "tile":   # one whole 64-key tile padded inside the valid range
        mask[:, 64:128] = True
    return mask


@pytest.mark.parametrize("mask_kind", ["none", "ragged", "tile"])
@pytest.mark.parametrize("B,S,H,heads", [(2, 64, 256, 2), (3, 70, 256, 2), (2, 130, 256, 4), (1, 257, 1024, 8)])
def test_attention(B, S, H, heads, mask_kind):
    if mask_kind == "tile" and S < 130:
        mask = _mask("none", B, S)
        mask[:, :min(S, 64) - 3] = True   # the first 64-key tile all but padded: the valid keys start late
    else:
        mask = _mask(mask_kind, B, S)
    qkv = rnd(B * S, 3 * H, seed=10)
    ref = _attn_ref(r16(qkv), mask, B, S, H, heads)
    got = G.attention(F16, qkv, mask, B, S, H, heads).float()
    err = float((got - ref).abs().max())
    assert err <= tol(ref, 2.5e-3), (err, tol(ref, 2.5e-3))   # bf16's bound here is 2e-2 (q, p AND the output are rounded)


def test_attention_spike_forces_rescale():
    """One key dominates late in the row: its score exceeds the running maximum by ~68 nats (2^98), far past what a binary16
    softmax numerator could hold against a stale maximum (2^16).  The online rescale keeps every numerator <= 2^6."""
    B, S, H, heads = 1, 256, 256, 2
    qkv = rnd(B * S, 3 * H, seed=12)
    qkv[200, H:H + 128] = 6.0 * qkv[5, :128]  # key 200 aligned with query 5 (head 0)
    mask = torch.zeros(B, S, dtype=torch.bool)
    ref = _attn_ref(r16(qkv), mask, B, S, H, heads)
    got = G.attention(F16, qkv, mask, B, S, H, heads).float()
    assert bool(torch.isfinite(got).all())
    assert float((got - ref).abs().max()) <= tol(ref, 2.5e-3)
    assert float((got[5, :128] - r16(qkv)[200, 2 * H:2 * H + 128]).abs().max()) <= tol(ref, 2.5e-3)   # query 5 attends to key 200 alone


@pytest.mark.parametrize("B,S,mask_kind", [(2, 40, "ragged"), (3, 130, "ragged"), (2, 257, "tile"), (3, 1, "none")])
def test_attention_out_projection_layernorm_one_launch(B, S, mask_kind):
    """attn_out_ln_kernel<f16> (the decoder's attention block of the H = 256, two-head architectures up to 768 frames) against torch
    and against the two launches it replaces; the bf16 test's bounds with the roundoff scaled by 2^-3."""
    H, heads = 256, 2
    qkv = rnd(B * S, 3 * H, seed=10)
    w, bias = rnd(H, H, seed=12, scale=H ** -0.5), 0.3 * rnd(H, seed=13)
    res = rnd(B * S, H, seed=14)
    g, be = 1 + 0.2 * rnd(H, seed=15), 0.1 * rnd(H, seed=16)
    mask = _mask(mask_kind, B, S)
    att = r16(_attn_ref(r16(qkv), mask, B, S, H, heads))
    ref = F.layer_norm(r16(res) + att @ r16(w).T + bias, (H,), g, be, 1e-5)
    got = G.attn_out_ln(qkv, mask, w, bias, res, g, be, B, S, H, heads, dtype=F16, raw=True)
    assert not torch.isnan(got).any()
    assert float((got.float() - ref).abs().max()) <= 5e-3 * (float(ref.abs().max()) + 1)
    two = G.gemm_ln(F16, G.attention(F16, qkv, mask, B, S, H, heads), w, bias, res, g, be)[0]
    assert float((got.float() - two).abs().max()) <= 2.5e-3 * (float(two.abs().max()) + 1)    # one f16 ulp of an O(1) value at most
    assert float((got.float() - two).abs().mean()) <= 1.25e-4
    assert torch.equal(G.attn_out_ln(qkv, mask, w, bias, res, g, be, B, S, H, heads, dtype=F16, raw=True).view(torch.int16), got.view(torch.int16))


# ---- row kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 9, 17])
@pytest.mark.parametrize("B,S,C_", [(2, 70, 256), (1, 300, 768)])
def test_dwconv(B, S, C_, k):
    x, w, b = rnd(B, S, C_, seed=18), rnd(C_, 1, k, seed=19, scale=k ** -0.5), rnd(C_, seed=20)
    ref = F.conv1d(r16(x).transpose(1, 2), w, b, padding="same", groups=C_).transpose(1, 2)
    got = G.dwconv(F16, x.reshape(B * S, C_), w, b, B, S).float().reshape(B, S, C_)
    assert float((got - ref).abs().max()) <= tol(ref)


@pytest.mark.parametrize("k", [3, 9, 17])
def test_dwconv_tile_heights_are_bit_identical(k):
    """An utterance gives the same bits alone (128-row tiles) and inside a batch of 64 (256-row tiles)."""
    B, S, C_ = 64, 300, 256
    x, w, b = rnd(B, S, C_, seed=180), rnd(C_, 1, k, seed=190, scale=k ** -0.5), rnd(C_, seed=200)
    whole = G.dwconv(F16, x.reshape(B * S, C_), w, b, B, S, raw=True).reshape(B, S, C_)
    alone = G.dwconv(F16, x[5:6].reshape(S, C_), w, b, 1, S, raw=True).reshape(1, S, C_)
    assert torch.equal(alone.view(torch.int16), whole[5:6].contiguous().view(torch.int16))
    ref = F.conv1d(r16(x[:2]).transpose(1, 2), w, b, padding="same", groups=C_).transpose(1, 2)
    assert float((whole[:2].float() - ref).abs().max()) <= tol(ref)


@pytest.mark.parametrize("M", [5, 300])
@pytest.mark.parametrize("Hd", [256, 768])
def test_layernorm_residual_and_head(M, Hd):
    x, r = rnd(M, Hd, seed=13, scale=2.0), rnd(M, Hd, seed=14)
    g, b = 1 + 0.2 * rnd(Hd, seed=15), 0.1 * rnd(Hd, seed=16)
    w = rnd(Hd, seed=17, scale=Hd ** -0.5)
    mask = torch.zeros(M, dtype=torch.bool)
    mask[::3] = True
    ref = F.layer_norm(r16(x) + r16(r), (Hd,), g, b, 1e-5)
    y, pred = G.layernorm(F16, x, r, g, b, dot_w=w, dot_b=0.25, mask=mask)
    assert float((y.float() - ref).abs().max()) <= tol(ref)
    pref = (ref @ w + 0.25).masked_fill(mask, 0)
    assert float((pred - pref).abs().max()) <= 5e-5 * (float(pref.abs().max()) + 1)
    y2, _ = G.layernorm(F16, x, None, g, b)
    ref2 = F.layer_norm(r16(x), (Hd,), g, b, 1e-5)
    assert float((y2.float() - ref2).abs().max()) <= tol(ref2)


# ---- what does not take the type says so ---------------------------------------------------------------------------------------
def test_operators_without_an_f16_form_reject_it():
    """Valid small buffers, FS2_F16 as the dtype: an error status before anything is launched (0 from the *_supported query)."""
    lib, st = G.lib(), torch.cuda.current_stream()
    dv = G.DEV
    B, S, Hd = 2, 8, 256
    x = torch.zeros(B * S, Hd, dtype=T16, device=dv)
    y = torch.full((B * S, Hd), 7.0, dtype=T16, device=dv)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dv)
    assert lib.fs2_op_attention_bwd_supported(F16, 256, 2) == 0
    d = _lib.BGemmDescC()
    for k, v in dict(M=16, N=16, K=16, sAm=16, sAk=1, sBk=16, sBn=1, ldc=16, nb1=1, nb2=1, alpha=1.0, beta=0.0, splitk=1, taps=1, c_dtype=F16).items():
        setattr(d, k, v)
    a16 = torch.zeros(16, 16, dtype=T16, device=dv)
    assert lib.fs2_op_bgemm(F16, C.byref(d), a16, a16, a16.clone(), None, None, st) != 0
    w = torch.zeros(2, Hd, 3 * Hd, dtype=T16, device=dv)
    scratch = torch.zeros(2 * Hd * 3 * Hd * 2, dtype=torch.uint8, device=dv)
    assert lib.fs2_op_predictor(F16, x, w, f32(2, Hd), f32(2, Hd), f32(2, Hd), f32(Hd), 0.0, None, f32(B * S), scratch, B, S, Hd, 2, 3, st) != 0
    cum = torch.tensor([[1, 2, 3, 4]] * B, dtype=torch.int32, device=dv)
    tot = torch.tensor([4] * B, dtype=torch.int32, device=dv)
    xs = torch.zeros(B * 4, Hd, dtype=T16, device=dv)
    mk = torch.zeros(B, 4, dtype=torch.uint8, device=dv)
    assert lib.fs2_op_regulate(F16, xs, cum, tot, y, mk, B, 4, 4, Hd, st) != 0
    idx = torch.zeros(B * S, dtype=torch.int32, device=dv)
    assert lib.fs2_op_bucket_embed(F16, x, f32(B * S), f32(3), f32(4, Hd), 4, 1.0, 0.0, None, None, y, idx, B, S, Hd, st) != 0
    ph = torch.ones(B, S, dtype=torch.int64, device=dv)
    smk = torch.zeros(B, S, dtype=torch.uint8, device=dv)
    assert lib.fs2_op_embed(F16, ph, f32(10, Hd), f32(S, Hd), f32(B, Hd), y, smk, B, S, Hd, 10, st) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())   # nothing was written
