"""Helpers for the `-m gpu` parity tests: call single operators of libfs2_hip.so through the C ABI."""
import ctypes as C

import numpy as np
import torch

import _f16
from lightningfastspeech2_amd import _lib

F32, BF16, F16 = _lib.FS2_F32, _lib.FS2_BF16, _lib.FS2_F16
_TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DEV = "cuda:0"


def lib():
    return _lib.load()


def ok(status, what=""):
    assert status == 0, f"{what}: status {status} ({lib().fs2_status_string(status).decode()})"


def to_dev(x, dtype):
    """fp32 host/torch tensor -> device tensor in the storage dtype, by the storage rule of _f16.store."""
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return _f16.store(t, _TDT[dtype]).to(DEV).contiguous()


def tdt(dtype):
    return _TDT[dtype]


def rounded(x, dtype):
    """What the kernel actually sees: fp32 value of the (possibly 16-bit-rounded) input."""
    return _f16.rnd16(torch.as_tensor(x).float(), _TDT[dtype])


def host(t, raw=False):
    """a device result on the host: widened to fp32, or (raw) in its storage dtype, for tests that compare bit patterns"""
    return None if t is None else t.cpu() if raw else t.float().cpu()


def convert(src_dtype, dst_dtype, src):
    """fs2_op_convert on a device tensor -> a device tensor"""
    out = torch.empty(src.shape, dtype=tdt(dst_dtype), device=DEV)
    ok(lib().fs2_op_convert(src_dtype, dst_dtype, src, out, src.numel(), torch.cuda.current_stream()), "convert")
    torch.cuda.synchronize()
    return out


def gemm(dtype, x, w_packed, bias, taps=1, S=None, relu=False, out_dtype=None, raw=False):
    M, Cin = x.shape
    N = w_packed.shape[0]
    out_dtype = dtype if out_dtype is None else out_dtype
    xd, wd = to_dev(x, dtype), to_dev(w_packed, dtype)
    bd = None if bias is None else torch.as_tensor(bias).float().to(DEV)
    c = torch.empty(M, N, dtype=tdt(out_dtype), device=DEV)
    ok(lib().fs2_op_gemm(dtype, out_dtype, xd, wd, bd, c, M, N, Cin, taps, S or M, int(relu), torch.cuda.current_stream()), "gemm")
    torch.cuda.synchronize()
    return host(c, raw)


def gemm_add(dtype, x, w_packed, bias, addend, taps=1, S=None, in_place=True, raw=False):
    M, Cin = x.shape
    N = w_packed.shape[0]
    xd, wd, ad = to_dev(x, dtype), to_dev(w_packed, dtype), to_dev(addend, dtype)
    bd = None if bias is None else torch.as_tensor(bias).float().to(DEV)
    c = ad if in_place else torch.empty(M, N, dtype=tdt(dtype), device=DEV)
    ok(lib().fs2_op_gemm_add(dtype, xd, wd, bd, ad, c, M, N, Cin, taps, S or M, torch.cuda.current_stream()), "gemm_add")
    torch.cuda.synchronize()
    return host(c, raw)


def gemm_rowscale(x, w_folded, bias_folded, parts, wg, eps=1e-5):
    """fs2_op_rowstats_finish + fs2_op_gemm_rowscale (bf16): x = pre-norm rows, parts (M, nparts, 2) fp32 partial (sum, sum of
    squares) per row as the deferred-LayerNorm epilogue leaves them"""
    M, Cin = x.shape
    N = w_folded.shape[0]
    xd, wd = to_dev(x, BF16), to_dev(w_folded, BF16)
    bd = torch.as_tensor(bias_folded).float().to(DEV).contiguous()
    sd = torch.as_tensor(parts).float().to(DEV).contiguous()
    gd = torch.as_tensor(wg).float().to(DEV).contiguous()
    rs = torch.empty(M, 2, dtype=torch.float32, device=DEV)
    ok(lib().fs2_op_rowstats_finish(sd, int(parts.shape[1]), Cin, eps, rs, M, torch.cuda.current_stream()), "rowstats_finish")
    c = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ok(lib().fs2_op_gemm_rowscale(xd, wd, bd, rs, gd, c, M, N, Cin, torch.cuda.current_stream()), "gemm_rowscale")
    torch.cuda.synchronize()
    return c.float().cpu()


def gemm_stats(dtype, x, w, bias, res, relu=False):
    """fs2_op_gemm_stats: the deferred-LayerNorm epilogue -> (v (M, N) in dtype, stats (M, ceil(N / 256), 2) fp32), both left on the device."""
    M, Cin = x.shape
    N = w.shape[0]
    xd, wd, bd = to_dev(x, dtype), to_dev(w, dtype), to_dev(bias, F32)
    rd = None if res is None else to_dev(res, dtype)
    v = torch.empty(M, N, dtype=tdt(dtype), device=DEV)
    st = torch.full((M, (N + 255) // 256, 2), float("nan"), dtype=torch.float32, device=DEV)
    ok(lib().fs2_op_gemm_stats(dtype, xd, wd, bd, rd, v, st, M, N, Cin, int(relu), torch.cuda.current_stream()), "gemm_stats")
    torch.cuda.synchronize()
    return v, st


def gemm_rowscale_dt(dtype, v_dev, stats_dev, w_folded, bias_folded, wg, out_dtype=None, eps=1e-5):
    """fs2_op_rowstats_finish + fs2_op_gemm_rowscale_dt on device tensors as gemm_stats left them; the result in out_dtype."""
    M, Cin = v_dev.shape
    N = w_folded.shape[0]
    out_dtype = dtype if out_dtype is None else out_dtype
    wd, bd, gd = to_dev(w_folded, dtype), to_dev(bias_folded, F32), to_dev(wg, F32)
    rs = torch.empty(M, 2, dtype=torch.float32, device=DEV)
    ok(lib().fs2_op_rowstats_finish(stats_dev, int(stats_dev.shape[1]), Cin, eps, rs, M, torch.cuda.current_stream()), "rowstats_finish")
    c = torch.empty(M, N, dtype=tdt(out_dtype), device=DEV)
    ok(lib().fs2_op_gemm_rowscale_dt(dtype, out_dtype, v_dev, wd, bd, rs, gd, c, M, N, Cin, torch.cuda.current_stream()), "gemm_rowscale_dt")
    torch.cuda.synchronize()
    return c.cpu()


def gemm_head(x, w, bias, gamma, beta, w_head, b_head, mask=None, relu=True, eps=1e-5):
    """fs2_op_gemm_head + fs2_op_head_finish (bf16): pred = masked(LayerNorm(act(x w^T + bias)) . w_head + b_head) from the epilogue's
    row sums; also returns the statistic parts (M, nparts, 2) and the head sums (M, nparts)"""
    M, Cin = x.shape
    N = w.shape[0]
    nparts = (N + 255) // 256
    xd, wd = to_dev(x, BF16), to_dev(w, BF16)
    bd = torch.as_tensor(bias).float().to(DEV).contiguous()
    gw = (torch.as_tensor(gamma).float() * torch.as_tensor(w_head).float())
    gd = gw.to(DEV).contiguous()
    st = torch.full((M, nparts, 2), float("nan"), dtype=torch.float32, device=DEV)
    hd = torch.full((M, nparts), float("nan"), dtype=torch.float32, device=DEV)
    ok(lib().fs2_op_gemm_head(xd, wd, bd, gd, st, hd, M, N, Cin, int(relu), torch.cuda.current_stream()), "gemm_head")
    md = None if mask is None else torch.as_tensor(mask).to(torch.uint8).to(DEV).contiguous()
    pred = torch.empty(M, dtype=torch.float32, device=DEV)
    cst = float((torch.as_tensor(beta).double() * torch.as_tensor(w_head).double()).sum() + b_head)
    ok(lib().fs2_op_head_finish(st, hd, nparts, N, eps, gw.double().sum(), cst, md, pred, M, torch.cuda.current_stream()), "head_finish")
    torch.cuda.synchronize()
    return pred.cpu(), st.cpu(), hd.cpu()


def gemm_splitk(dtype, x, w_packed, ksplit, taps=1, S=None, out_dtype=None, into=None):
    """fs2_op_gemm_splitk: K slices as workgroups of one launch into fp32 planes + the plane sum; into = a tensor the result is
    ADDED to (the accumulating data-gradient call of the training step)."""
    M, Cin = x.shape
    N = w_packed.shape[0]
    out_dtype = dtype if out_dtype is None else out_dtype
    xd, wd = to_dev(x, dtype), to_dev(w_packed, dtype)
    c = torch.empty(M, N, dtype=tdt(out_dtype), device=DEV) if into is None else to_dev(into, out_dtype).clone()
    part = torch.empty(ksplit, M, N, dtype=torch.float32, device=DEV)
    ok(lib().fs2_op_gemm_splitk(dtype, out_dtype, xd, wd, c, part, M, N, Cin, taps, S or M, ksplit, int(into is not None),
                                torch.cuda.current_stream()), "gemm_splitk")
    torch.cuda.synchronize()
    return c.float().cpu()


def gemm_ln(dtype, x, w_packed, bias, res, g, b, taps=1, S=None, relu=False, dot_w=None, dot_b=0.0, mask=None, want_y=True, raw=False):
    M, Cin = x.shape
    N = w_packed.shape[0]
    f = lambda a: None if a is None else torch.as_tensor(a).float().to(DEV).contiguous()
    xd, wd = to_dev(x, dtype), to_dev(w_packed, dtype)
    rd = None if res is None else to_dev(res, dtype)
    y = torch.empty(M, N, dtype=tdt(dtype), device=DEV) if want_y else None
    tmp = torch.empty(M, N, dtype=tdt(dtype), device=DEV)
    pred = torch.empty(M, dtype=torch.float32, device=DEV) if dot_w is not None else None
    mk = None if mask is None else torch.as_tensor(mask).to(torch.uint8).to(DEV)
    bd, gd, bed, dwd = f(bias), f(g), f(b), f(dot_w)
    ok(lib().fs2_op_gemm_ln(dtype, xd, wd, bd, rd, gd, bed, dwd, dot_b, mk, pred, y, tmp, M, N, Cin, taps, S or M, int(relu),
                            torch.cuda.current_stream()), "gemm_ln")
    torch.cuda.synchronize()
    return host(y, raw), host(pred)


def predictor(x, ws, biases, gammas, betas, head_w, head_b, mask, B, S):
    """Single-launch VariancePredictor (bf16): ws = list of (H, H, k) conv weights (torch layout)."""
    H, nl, k = x.shape[-1], len(ws), ws[0].shape[2]
    xd = to_dev(x.reshape(B * S, H), BF16)
    wd = to_dev(torch.stack([pack_conv_weight(w) for w in ws]), BF16)
    f = lambda a: torch.stack([torch.as_tensor(v).float() for v in a]).to(DEV).contiguous()
    bd, gd, bed = f(biases), f(gammas), f(betas)
    hw = torch.as_tensor(head_w).float().to(DEV)
    mk = None if mask is None else torch.as_tensor(mask).to(torch.uint8).to(DEV).contiguous()
    pred = torch.full((B * S,), float("nan"), dtype=torch.float32, device=DEV)
    scratch = torch.empty(nl * H * k * H * 2, dtype=torch.uint8, device=DEV)
    ok(lib().fs2_op_predictor(BF16, xd, wd, bd, gd, bed, hw, head_b, mk, pred, scratch, B, S, H, nl, k, torch.cuda.current_stream()), "predictor")
    torch.cuda.synchronize()
    return pred.cpu().reshape(B, S)


def predictor_dw(x, dws, dwbs, ws, biases, gammas, betas, head_w, head_b, mask, B, S):
    """Single-launch depth-wise VariancePredictor (bf16): dws = list of (H, 1, 3) depth-wise weights, ws = list of (H, H, 1) pointwise."""
    H, nl = x.shape[-1], len(ws)
    xd = to_dev(x.reshape(B * S, H), BF16)
    wd = to_dev(torch.stack([w.reshape(H, H) for w in ws]), BF16)
    f = lambda a: torch.stack([torch.as_tensor(v).float() for v in a]).to(DEV).contiguous()
    dwd = f([w.reshape(H, 3).t().contiguous() for w in dws])   # (nl, 3, H) tap-major
    dbd, bd, gd, bed = f(dwbs), f(biases), f(gammas), f(betas)
    hw = torch.as_tensor(head_w).float().to(DEV)
    mk = None if mask is None else torch.as_tensor(mask).to(torch.uint8).to(DEV).contiguous()
    pred = torch.full((B * S,), float("nan"), dtype=torch.float32, device=DEV)
    scratch = torch.empty(nl * H * H * 2, dtype=torch.uint8, device=DEV)
    ok(lib().fs2_op_predictor_dw(BF16, xd, dwd, dbd, wd, bd, gd, bed, hw, head_b, mk, pred, scratch, B, S, H, nl,
                                 torch.cuda.current_stream()), "predictor_dw")
    torch.cuda.synchronize()
    return pred.cpu().reshape(B, S)


def pack_conv_weight(w):
    """torch (N, Cin, k) -> (N, k*Cin) tap-major (what the engine builds at fs2_finalize)."""
    w = torch.as_tensor(w).float()
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def attention(dtype, qkv, key_pad_mask, B, S, H, heads, raw=False):
    qd = to_dev(qkv, dtype)
    md = torch.as_tensor(key_pad_mask).to(torch.uint8).to(DEV).contiguous()
    out = torch.empty(B * S, H, dtype=tdt(dtype), device=DEV)
    bits_bytes = C.c_size_t()
    vt_bytes = lib().fs2_op_attention_scratch_bytes(dtype, B, S, H, heads, C.byref(bits_bytes))
    vt = torch.empty(vt_bytes, dtype=torch.uint8, device=DEV)
    bits = torch.empty(bits_bytes.value, dtype=torch.uint8, device=DEV)
    ok(lib().fs2_op_attention(dtype, qd, md, out, vt, bits, B, S, H, heads, torch.cuda.current_stream()), "attention")
    torch.cuda.synchronize()
    return host(out, raw)


def attn_out_ln(qkv, key_pad_mask, w_out, bias, res, gamma, beta, B, S, H, heads, dtype=BF16, raw=False):
    """fs2_op_attn_out_ln (16-bit storage): LayerNorm(res + MHA-core(qkv) w_out^T + bias)."""
    qd, rd, wd = to_dev(qkv, dtype), to_dev(res, dtype), to_dev(w_out, dtype)
    md = torch.as_tensor(key_pad_mask).to(torch.uint8).to(DEV).contiguous()
    f = lambda v: torch.as_tensor(v).float().to(DEV).contiguous()
    bd, gd, bed = f(bias), f(gamma), f(beta)
    out = torch.empty(B * S, H, dtype=tdt(dtype), device=DEV)
    scratch = torch.empty(H * H * 2 + B * ((S + 63) // 64) * 8, dtype=torch.uint8, device=DEV)
    ok(lib().fs2_op_attn_out_ln(dtype, qd, md, wd, bd, rd, gd, bed, out, scratch, B, S, H, heads, torch.cuda.current_stream()), "attn_out_ln")
    torch.cuda.synchronize()
    return host(out, raw)


def attention_x3(qkv, key_pad_mask, B, S, H, heads):
    """fs2_op_attention_x3: fp32 qkv, bf16 x 3 split products, fp32 out."""
    qd = torch.as_tensor(qkv).float().to(DEV).contiguous()
    md = torch.as_tensor(key_pad_mask).to(torch.uint8).to(DEV).contiguous()
    out = torch.empty(B * S, H, dtype=torch.float32, device=DEV)
    split = torch.empty(2 * B * S * 3 * H, dtype=torch.bfloat16, device=DEV)
    bits = torch.empty(B * ((S + 63) // 64) * 8, dtype=torch.uint8, device=DEV)
    ok(lib().fs2_op_attention_x3(qd, md, out, split, bits, B, S, H, heads, torch.cuda.current_stream()), "attention_x3")
    torch.cuda.synchronize()
    return out.cpu()


def gemm_split_out(x, w, bias, split=True):
    M, K = x.shape
    N = w.shape[0]
    xd, wd = torch.as_tensor(x).float().to(DEV).contiguous(), torch.as_tensor(w).float().to(DEV).contiguous()
    bd = None if bias is None else torch.as_tensor(bias).float().to(DEV)
    hi = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    lo = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ok(lib().fs2_op_gemm_split_out(xd, wd, bd, hi, lo, M, N, K, int(split), torch.cuda.current_stream()), "gemm_split_out")
    torch.cuda.synchronize()
    return hi.float().cpu(), lo.float().cpu()


def layernorm(dtype, x, res, gamma, beta, dot_w=None, dot_b=0.0, mask=None, want_y=True, raw=False):
    M, H = x.shape
    xd = to_dev(x, dtype)
    rd = None if res is None else to_dev(res, dtype)
    g, b = torch.as_tensor(gamma).float().to(DEV), torch.as_tensor(beta).float().to(DEV)
    y = torch.empty(M, H, dtype=tdt(dtype), device=DEV) if want_y else None
    dw = None if dot_w is None else torch.as_tensor(dot_w).float().to(DEV)
    mk = None if mask is None else torch.as_tensor(mask).to(torch.uint8).to(DEV)
    pred = torch.empty(M, dtype=torch.float32, device=DEV) if dot_w is not None else None
    ok(lib().fs2_op_layernorm(dtype, xd, rd, g, b, y, dw, dot_b, mk, pred, M, H, torch.cuda.current_stream()), "layernorm")
    torch.cuda.synchronize()
    return host(y, raw), host(pred)


def dwconv(dtype, x, w, bias, B, S, raw=False):
    C_ = x.shape[1]
    k = w.shape[-1]
    xd = to_dev(x, dtype)
    wd = torch.as_tensor(w).float().reshape(C_, k).to(DEV).contiguous()
    bd = torch.as_tensor(bias).float().to(DEV)
    y = torch.empty(B * S, C_, dtype=tdt(dtype), device=DEV)
    ok(lib().fs2_op_dwconv(dtype, xd, wd, bd, y, B, S, C_, k, torch.cuda.current_stream()), "dwconv")
    torch.cuda.synchronize()
    return host(y, raw)


# ------------------------------------------------------------------------------------------------
# Sentinel-filled outputs: a row the kernel never writes, or a write past the end, shows up instead of passing by the luck of what
# torch.empty handed out.  x_s returns (status, buffers...) and never raises on a status (tests/test_gpu_decisions.py); the plain x
# is x_s + ok(status), with the guard rows cut off and the results on the host.
def sentinel(rows, width, dtype):
    """(rows + 1, width) device buffer: floats NaN, integers / masks bytes of 0x5a; the last row is the guard row."""
    if dtype in (torch.float32, torch.bfloat16):
        return torch.full((rows + 1, width), float("nan"), dtype=dtype, device=DEV)
    t = torch.empty((rows + 1, width), dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0x5A)
    return t


def bits(t):
    """Raw bits of a float tensor (bf16, f16 -> int16, fp32 -> int32) on the host: equality of these is bit equality."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def to_bits(x, dtype):
    """fp32 reference values -> the bits they have in the engine dtype (one round-to-nearest-even for bf16)."""
    return bits(torch.as_tensor(x).float().to(tdt(dtype)))


def guard_intact(buf):
    """The guard row behind the end still holds the sentinel."""
    fresh = sentinel(0, buf.shape[1], buf.dtype)
    return torch.equal(buf[-1:].contiguous().view(torch.uint8).cpu(), fresh.view(torch.uint8).cpu())


def untouched(buf):
    """Every byte of the buffer still holds the sentinel (an op that declined its shape wrote nothing)."""
    fresh = sentinel(buf.shape[0] - 1, buf.shape[1], buf.dtype)
    return torch.equal(buf.view(torch.uint8).cpu(), fresh.view(torch.uint8).cpu())


def durations_s(dur_pred, src_mask, forced=None):
    """-> status, dur, cum (B, L) int32, totals, guard (B,) int32, all guard rows intact?"""
    B, L = dur_pred.shape
    dp = torch.as_tensor(dur_pred).float().to(DEV).contiguous()
    mk = torch.as_tensor(src_mask).to(torch.uint8).to(DEV).contiguous()
    fd = None if forced is None else torch.as_tensor(forced).to(torch.int32).to(DEV).contiguous()
    dur, cum = sentinel(B, L, torch.int32), sentinel(B, L, torch.int32)
    tot, grd = sentinel(B, 1, torch.int32), sentinel(B, 1, torch.int32)
    st = lib().fs2_op_durations(dp, mk, fd, dur, cum, tot, grd, B, L, torch.cuda.current_stream())
    torch.cuda.synchronize()
    intact = all(guard_intact(b) for b in (dur, cum, tot, grd))
    return st, dur[:B].cpu(), cum[:B].cpu(), tot[:B, 0].cpu(), grd[:B, 0].cpu(), intact


def durations(dur_pred, src_mask, forced=None):
    st, *out, _ = durations_s(dur_pred, src_mask, forced)
    ok(st, "durations")
    return tuple(out)


def regulate_s(dtype, x, cum, totals, B, L, T, H):
    """-> status, y buffer (B*T + 1, H) on the device, mask buffer (B + 1, T) uint8 on the device (raw bytes)."""
    xd = to_dev(x, dtype)
    cd = torch.as_tensor(cum).to(torch.int32).to(DEV).contiguous()
    td = torch.as_tensor(totals).to(torch.int32).to(DEV).contiguous()
    y, mk = sentinel(B * T, H, tdt(dtype)), sentinel(B, T, torch.uint8)
    st = lib().fs2_op_regulate(dtype, xd, cd, td, y, mk, B, L, T, H, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, y, mk


def regulate(dtype, x, cum, totals, B, L, T, H):
    st, y, mk = regulate_s(dtype, x, cum, totals, B, L, T, H)
    ok(st, "regulate")
    return y[:-1].float().cpu(), mk[:-1].bool().cpu()


def bucket_embed_s(entry, dtype, x, src, bins, emb, std, mean, pe, spk, B, T, H):
    """entry: "row" (fs2_op_bucket_embed), "utt" (fs2_op_bucket_embed_utt: src (B,), std 1, mean 0, no pe / spk) or "target"
    (fs2_op_bucket_embed_target).  -> status, y buffer (B*T + 1, H), idx buffer (B*T + 1, 1) int32, both on the device."""
    xd = to_dev(x, dtype)
    f = lambda a: None if a is None else torch.as_tensor(a).float().to(DEV).contiguous()
    sd, bd, ed, ped, spd = f(src), f(bins), f(emb), f(pe), f(spk)
    nb = 0 if emb is None else emb.shape[0]
    y, idx = sentinel(B * T, H, tdt(dtype)), sentinel(B * T, 1, torch.int32)
    if entry == "utt":
        assert std == 1.0 and mean == 0.0 and pe is None and spk is None
        st = lib().fs2_op_bucket_embed_utt(dtype, xd, sd, bd, ed, nb, y, idx, B, T, H, torch.cuda.current_stream())
    else:
        fn = lib().fs2_op_bucket_embed if entry == "row" else lib().fs2_op_bucket_embed_target
        st = fn(dtype, xd, sd, bd, ed, nb, std, mean, ped, spd, y, idx, B, T, H, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, y, idx


def bucket_embed(dtype, x, pred, bins, emb, std, mean, pe, spk, B, T, H):
    st, y, idx = bucket_embed_s("row", dtype, x, pred, bins, emb, std, mean, pe, spk, B, T, H)
    ok(st, "bucket_embed")
    return y[:-1].float().cpu(), idx[:-1, 0].cpu()


def embed_s(dtype, phones, table, pe, spk, n_phones):
    """-> status, x buffer (B*L + 1, H), src_mask buffer (B + 1, L) uint8, on the device."""
    B, L = phones.shape
    H = table.shape[1]
    ph = torch.as_tensor(phones).long().to(DEV).contiguous()
    f = lambda a: torch.as_tensor(a).float().to(DEV).contiguous()
    td, ped, sd = f(table), f(pe), f(spk)
    x, mk = sentinel(B * L, H, tdt(dtype)), sentinel(B, L, torch.uint8)
    st = lib().fs2_op_embed(dtype, ph, td, ped, sd, x, mk, B, L, H, n_phones, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, x, mk


def embed(dtype, phones, table, pe, spk, n_phones):
    st, x, mk = embed_s(dtype, phones, table, pe, spk, n_phones)
    ok(st, "embed")
    return x[:-1].float().cpu(), mk[:-1].bool().cpu()


def spk_proj_s(dvec, w, b):
    """-> status, out buffer (B + 1, H) fp32 on the device."""
    B, Din = dvec.shape
    H = w.shape[0]
    f = lambda a: torch.as_tensor(a).float().to(DEV).contiguous()
    dd, wd, bd = f(dvec), f(w), f(b)
    out = sentinel(B, H, torch.float32)
    st = lib().fs2_op_spk_proj(dd, wd, bd, out, B, H, Din, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, out


def spk_proj(dvec, w, b):
    st, out = spk_proj_s(dvec, w, b)
    ok(st, "spk_proj")
    return out[:-1].cpu()


def cwt_head_s(dtype, out_conv, spec, mask, ms_w, ms_b, B, T, F):
    """fs2_op_cwt_head: out_conv (B*T, F), spec (B*T, ld_spec) -> status, mean_std (B + 1, 2), pred (B + 1, T), spec_out (B*T + 1, 10) buffers."""
    od = to_dev(out_conv, dtype)
    f = lambda a: torch.as_tensor(a).float().to(DEV).contiguous()
    sd, wd, bd = f(spec), f(ms_w), f(ms_b)
    md = None if mask is None else torch.as_tensor(mask).to(torch.uint8).to(DEV).contiguous()
    ms, pred, so = sentinel(B, 2, torch.float32), sentinel(B, T, torch.float32), sentinel(B * T, 10, torch.float32)
    st = lib().fs2_op_cwt_head(dtype, od, sd, int(spec.shape[1]), md, wd, bd, ms, pred, so, B, T, F, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, ms, pred, so


# ------------------------------------------------------------------------------------------------
# The training tape's launches (tests/test_gpu_tape_ops.py), in the x_s convention: (status, sentinel buffers...), never raising.
def _f32(a):
    return None if a is None else torch.as_tensor(a).float().to(DEV).contiguous()


def _u8(a):
    return None if a is None else torch.as_tensor(a).to(torch.uint8).to(DEV).contiguous()


def dropout_keep(shape, p, seed, key):
    """fs2_op_dropout on fp32 ones of `shape`: the multiplier per element, 0 or the device's 1 / (1 - p), on the host."""
    ones = torch.ones(shape, dtype=torch.float32, device=DEV)
    out = torch.empty_like(ones)
    ok(lib().fs2_op_dropout(F32, ones, out, ones.numel(), p, C.c_uint64(seed), C.c_uint64(key), torch.cuda.current_stream()), "dropout")
    torch.cuda.synchronize()
    return out.cpu()


def gemm_ln_tape(dtype, x, w_packed, bias, res, g, b, taps, S, relu, drop=None, want_z=True):
    """fs2_op_gemm_ln_tape, or with drop = (p, seed, key) fs2_op_gemm_ln_tape_dropout -> status, y buffer, z buffer ((M + 1, N)
    sentinel buffers on the device; z None with want_z = False, which hands the entry a NULL z_out)."""
    M, Cin = x.shape
    N = w_packed.shape[0]
    xd, wd = to_dev(x, dtype), to_dev(w_packed, dtype)
    rd = None if res is None else to_dev(res, dtype)
    bd, gd, bed = _f32(bias), _f32(g), _f32(b)
    y = sentinel(M, N, tdt(dtype))
    z = sentinel(M, N, tdt(dtype)) if want_z else None
    if drop is None:
        st = lib().fs2_op_gemm_ln_tape(dtype, xd, wd, bd, rd, gd, bed, y, z, M, N, Cin, taps, S or M, int(relu), torch.cuda.current_stream())
    else:
        p, seed, key = drop
        st = lib().fs2_op_gemm_ln_tape_dropout(dtype, xd, wd, bd, rd, gd, bed, y, z, M, N, Cin, taps, S or M, int(relu), p,
                                               C.c_uint64(seed), C.c_uint64(key), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, y, z


def layernorm_bwd_s(dtype, z, res, dy, gamma, relu_mask, masked=None, want_dzm=True):
    """fs2_op_layernorm_bwd, or with masked = (out_p, seed, out_key) fs2_op_layernorm_bwd_masked -> status, dz buffer, dzm buffer
    (None for the plain entry or with want_dzm = False: a NULL dzm), part buffer (nparts * 3 + 1, H) fp32; z, res, dy are taken
    in the storage dtype by to_dev."""
    M, H = z.shape
    zd, dyd = to_dev(z, dtype), to_dev(dy, dtype)
    rd = None if res is None else to_dev(res, dtype)
    gd = _f32(gamma)
    nparts = lib().fs2_op_layernorm_bwd_parts(M)
    dz, part = sentinel(M, H, tdt(dtype)), sentinel(nparts * 3, H, torch.float32)
    dzm = None
    if masked is None:
        st = lib().fs2_op_layernorm_bwd(dtype, zd, rd, dyd, gd, dz, part, M, H, int(relu_mask), torch.cuda.current_stream())
    else:
        p, seed, key = masked
        dzm = sentinel(M, H, tdt(dtype)) if want_dzm else None
        st = lib().fs2_op_layernorm_bwd_masked(dtype, zd, rd, dyd, gd, dz, dzm, part, M, H, int(relu_mask), p, C.c_uint64(seed),
                                               C.c_uint64(key), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, dz, dzm, part


def layernorm_head_s(dtype, x, res, gamma, beta, dot_w, dot_b, mask, want_pred=True):
    """fs2_op_layernorm_head (the head's bias read from device memory; dot_w / dot_b None hand it a NULL) -> status, y buffer
    (M + 1, H), pred buffer (M + 1, 1) fp32 (None with want_pred = False)."""
    M, H = x.shape
    xd = to_dev(x, dtype)
    rd = None if res is None else to_dev(res, dtype)
    bdev = None if dot_b is None else torch.tensor([dot_b], dtype=torch.float32, device=DEV)
    y = sentinel(M, H, tdt(dtype))
    pred = sentinel(M, 1, torch.float32) if want_pred else None
    st = lib().fs2_op_layernorm_head(dtype, xd, rd, _f32(gamma), _f32(beta), y, _f32(dot_w), bdev, _u8(mask), pred, M, H,
                                     torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, y, pred


def row_dot_s(dtype, y, w, b, mask):
    """fs2_op_row_dot -> status, pred buffer (M + 1, 1) fp32 on the device."""
    M, H = y.shape
    yd = to_dev(y, dtype)
    bdev = torch.tensor([b], dtype=torch.float32, device=DEV)
    pred = sentinel(M, 1, torch.float32)
    st = lib().fs2_op_row_dot(dtype, yd, _f32(w), bdev, _u8(mask), pred, M, H, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st, pred
