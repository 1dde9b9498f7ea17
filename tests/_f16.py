"""Helpers of the FS2_F16 / precision="mixed16" tests.

(a) The storage rule on the host (`f16_round`, `f16_bits`), the edge-value vector the conversion tests share, and thin wrappers of the
    operator entry points that take FS2_F16 (tests/_gpu.py's know fp32 and bf16 only and stay as they are).
(b) `decoder_16bit`: a plain-torch CPU model of a decoder that STORES its tensors in a 16-bit type - the yardstick the end-to-end
    tests hold the engine's decoder to.  It restates what the engine rounds, nothing else: the matrix weights, the decoder input,
    qkv, the softmax numerators, the normalised attention output, both LayerNorm outputs, the depth-wise conv output and the
    post-ReLU FFN tensor go through the storage type; accumulation, softmax statistics, LayerNorm, biases and the depth-wise
    weights stay fp32.  Parameterised by torch.bfloat16 / torch.float16, so the same code models the "mixed3" and the "mixed16" back.
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from lightningfastspeech2_amd import _lib

F32, BF16, F16 = _lib.FS2_F32, _lib.FS2_BF16, _lib.FS2_F16
F16_MAX = 65504.0
DEV = "cuda:0"
_TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}


# ---- the storage rule ---------------------------------------------------------------------------------------------------------
def store(x, tdt):
    """fp32 -> what a store in `tdt` keeps, as a tensor of that type: binary16 saturates at +-65504 (NaN stays NaN), then both
    round to nearest-even."""
    x = torch.as_tensor(x).float()
    if tdt == torch.float16:
        x = torch.clamp(x, -F16_MAX, F16_MAX)
    return x.to(tdt)


def rnd16(x, tdt):
    """The fp32 value of what `store` keeps."""
    return x if tdt == torch.float32 else store(x, tdt).float()


def f16_bits(x):
    """Bits (int16) of the FS2_F16 storage of fp32 values, by the rule include/fs2.h states, in torch."""
    return store(x, torch.float16).contiguous().view(torch.int16)


def edge_values():
    """Every class of input the conversion has a branch for: normals at three scales, exact ties, the subnormal range, the largest
    finite value and what lies beyond it, signed zeros, infinities, NaN."""
    g = torch.Generator().manual_seed(5)
    parts = [torch.randn(4096, generator=g) * s for s in (1e-6, 1.0, 1e3)]
    k = torch.arange(0, 2048, dtype=torch.float32)
    parts.append((2048 + k + 0.5) * 2.0 ** -11)                    # ties between neighbours in [1, 2): even and odd below
    parts.append(-(2048 + k + 0.5) * 2.0 ** -5)                    # ... in [64, 128), negative
    parts.append((k + 0.5) * 2.0 ** -24)                           # ties between subnormals (and 0 | the smallest one)
    parts.append(torch.randn(4096, generator=g) * 2.0 ** -16)      # the subnormal range and the first normal binades
    parts.append(torch.tensor([2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -26, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12),
                               65504.0, -65504.0, 65519.9, 65520.0, -65520.0, 65535.0, 1e6, -1e6, 3e38, -3e38, 0.0, -0.0,
                               float("inf"), float("-inf"), float("nan")]))
    return torch.cat(parts).float().contiguous()


# ---- operator wrappers (device) -----------------------------------------------------------------------------------------------
def lib():
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ok(status, what=""):
    assert status == 0, f"{what}: status {status} ({lib().fs2_status_string(status).decode()})"


def dev(x, dt=F32):
    return store(x, _TDT[dt]).to(DEV).contiguous()


def f32dev(a):
    return None if a is None else torch.as_tensor(a).float().to(DEV).contiguous()


def convert(src_dt, dst_dt, src):
    out = torch.empty(src.shape, dtype=_TDT[dst_dt], device=DEV)
    ok(lib().fs2_op_convert(src_dt, dst_dt, p(src), p(out), src.numel(), stream()), "convert")
    torch.cuda.synchronize()
    return out


def gemm(x, w, bias, taps=1, S=None, relu=False, dt=F16, out_dt=None):
    M, Cin = x.shape
    N = w.shape[0]
    out_dt = dt if out_dt is None else out_dt
    xd, wd, bd = dev(x, dt), dev(w, dt), f32dev(bias)
    c = torch.empty(M, N, dtype=_TDT[out_dt], device=DEV)
    ok(lib().fs2_op_gemm(dt, out_dt, p(xd), p(wd), p(bd), p(c), M, N, Cin, taps, S or M, int(relu), stream()), "gemm")
    torch.cuda.synchronize()
    return c.cpu()


def gemm_add(x, w, bias, addend, dt=F16):
    M, Cin = x.shape
    N = w.shape[0]
    xd, wd, ad, bd = dev(x, dt), dev(w, dt), dev(addend, dt), f32dev(bias)
    c = torch.empty(M, N, dtype=_TDT[dt], device=DEV)
    ok(lib().fs2_op_gemm_add(dt, p(xd), p(wd), p(bd), p(ad), p(c), M, N, Cin, 1, M, stream()), "gemm_add")
    torch.cuda.synchronize()
    return c.cpu()


def gemm_stats(x, w, bias, res, relu=False, dt=F16):
    """fs2_op_gemm_stats: the deferred-LayerNorm epilogue -> (v (M, N) in dt, stats (M, ceil(N / 256), 2) fp32), both left on the device."""
    M, Cin = x.shape
    N = w.shape[0]
    xd, wd, bd = dev(x, dt), dev(w, dt), f32dev(bias)
    rd = None if res is None else dev(res, dt)
    v = torch.empty(M, N, dtype=_TDT[dt], device=DEV)
    st = torch.full((M, (N + 255) // 256, 2), float("nan"), dtype=torch.float32, device=DEV)
    ok(lib().fs2_op_gemm_stats(dt, p(xd), p(wd), p(bd), p(rd), p(v), p(st), M, N, Cin, int(relu), stream()), "gemm_stats")
    torch.cuda.synchronize()
    return v, st


def gemm_rowscale(v_dev, stats_dev, w_folded, bias_folded, wg, dt=F16, out_dt=None, eps=1e-5):
    """fs2_op_rowstats_finish + fs2_op_gemm_rowscale_dt on device tensors as gemm_stats left them."""
    M, Cin = v_dev.shape
    N = w_folded.shape[0]
    out_dt = dt if out_dt is None else out_dt
    wd, bd, gd = dev(w_folded, dt), f32dev(bias_folded), f32dev(wg)
    rs = torch.empty(M, 2, dtype=torch.float32, device=DEV)
    ok(lib().fs2_op_rowstats_finish(p(stats_dev), int(stats_dev.shape[1]), Cin, float(eps), p(rs), M, stream()), "rowstats_finish")
    c = torch.empty(M, N, dtype=_TDT[out_dt], device=DEV)
    ok(lib().fs2_op_gemm_rowscale_dt(dt, out_dt, p(v_dev), p(wd), p(bd), p(rs), p(gd), p(c), M, N, Cin, stream()), "gemm_rowscale_dt")
    torch.cuda.synchronize()
    return c.cpu()


def gemm_ln(x, w, bias, res, g, b, taps=1, S=None, relu=False, dt=F16):
    M, Cin = x.shape
    N = w.shape[0]
    xd, wd = dev(x, dt), dev(w, dt)
    rd = None if res is None else dev(res, dt)
    y = torch.empty(M, N, dtype=_TDT[dt], device=DEV)
    tmp = torch.empty(M, N, dtype=_TDT[dt], device=DEV)
    bd, gd, bed = f32dev(bias), f32dev(g), f32dev(b)
    ok(lib().fs2_op_gemm_ln(dt, p(xd), p(wd), p(bd), p(rd), p(gd), p(bed), None, 0.0, None, None, p(y), p(tmp), M, N, Cin, taps,
                            S or M, int(relu), stream()), "gemm_ln")
    torch.cuda.synchronize()
    return y.cpu()


def attention(qkv, key_pad_mask, B, S, H, heads, dt=F16):
    qd = dev(qkv, dt)
    md = torch.as_tensor(key_pad_mask).to(torch.uint8).to(DEV).contiguous()
    out = torch.empty(B * S, H, dtype=_TDT[dt], device=DEV)
    bits_bytes = C.c_size_t()
    vt_bytes = lib().fs2_op_attention_scratch_bytes(dt, B, S, H, heads, C.byref(bits_bytes))
    vt = torch.empty(max(vt_bytes, 16), dtype=torch.uint8, device=DEV)
    bits = torch.empty(bits_bytes.value, dtype=torch.uint8, device=DEV)
    ok(lib().fs2_op_attention(dt, p(qd), p(md), p(out), p(vt), p(bits), B, S, H, heads, stream()), "attention")
    torch.cuda.synchronize()
    return out.cpu()


def attn_out_ln(qkv, key_pad_mask, w_out, bias, res, gamma, beta, B, S, H, heads, dt=F16):
    qd, rd, wd = dev(qkv, dt), dev(res, dt), dev(w_out, dt)
    md = torch.as_tensor(key_pad_mask).to(torch.uint8).to(DEV).contiguous()
    bd, gd, bed = f32dev(bias), f32dev(gamma), f32dev(beta)
    out = torch.empty(B * S, H, dtype=_TDT[dt], device=DEV)
    scratch = torch.empty(H * H * 2 + B * ((S + 63) // 64) * 8, dtype=torch.uint8, device=DEV)
    ok(lib().fs2_op_attn_out_ln(dt, p(qd), p(md), p(wd), p(bd), p(rd), p(gd), p(bed), p(out), p(scratch), B, S, H, heads, stream()),
       "attn_out_ln")
    torch.cuda.synchronize()
    return out.cpu()


def layernorm(x, res, gamma, beta, dot_w=None, dot_b=0.0, mask=None, dt=F16):
    M, H = x.shape
    xd = dev(x, dt)
    rd = None if res is None else dev(res, dt)
    y = torch.empty(M, H, dtype=_TDT[dt], device=DEV)
    mk = None if mask is None else torch.as_tensor(mask).to(torch.uint8).to(DEV)
    pred = torch.empty(M, dtype=torch.float32, device=DEV) if dot_w is not None else None
    gd, bd, wd = f32dev(gamma), f32dev(beta), f32dev(dot_w)   # (named: a temporary's memory would be handed to the next allocation)
    ok(lib().fs2_op_layernorm(dt, p(xd), p(rd), p(gd), p(bd), p(y), p(wd), float(dot_b), p(mk), p(pred), M, H, stream()), "layernorm")
    torch.cuda.synchronize()
    return y.cpu(), (None if pred is None else pred.cpu())


def dwconv(x, w, bias, B, S, dt=F16):
    C_ = x.shape[1]
    k = w.shape[-1]
    xd = dev(x, dt)
    wd = torch.as_tensor(w).float().reshape(C_, k).to(DEV).contiguous()
    bd = f32dev(bias)
    y = torch.empty(B * S, C_, dtype=_TDT[dt], device=DEV)
    ok(lib().fs2_op_dwconv(dt, p(xd), p(wd), p(bd), p(y), B, S, C_, k, stream()), "dwconv")
    torch.cuda.synchronize()
    return y.cpu()


# ---- the 16-bit-storage decoder, on the CPU -----------------------------------------------------------------------------------
def decoder_16bit(sd, cfg, adaptor_out, speaker, tgt_mask, tdt):
    """mel (B, T, n_mels) fp32 of the decoder stack + mel Linear on the oracle's `adaptor_out`, storing in `tdt` what the engine
    stores (module docstring).  The depth-wise block's conv2 = grouped 1x1 conv, then pointwise, has no non-linearity in between:
    one linear map, folded in double and stored once, as the engine does at fs2_finalize."""
    from oracle import oracle_cpu as O
    r = lambda t: rnd16(t, tdt)
    H, heads = cfg.hidden, cfg.decoder_head
    d = H // heads
    spk = O.speaker_embedding(sd, torch.as_tensor(speaker).float())
    x = r(O.positional_encoding(torch.as_tensor(adaptor_out).float(), O._t(sd, "positional_encoding.pe")) + spk[:, None, :])
    B, T, _ = x.shape
    for i in range(cfg.decoder_layers):
        pfx = f"decoder.layers.{i}"
        t = lambda n: O._t(sd, f"{pfx}.{n}")
        qkv = r(F.linear(x, r(t("self_attn.in_proj_weight")), t("self_attn.in_proj_bias")))
        q, k, v = qkv.split(H, dim=-1)
        q = q.view(B, T, heads, d).transpose(1, 2) * (1.0 / math.sqrt(d))
        k = k.view(B, T, heads, d).transpose(1, 2)
        v = v.view(B, T, heads, d).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)).masked_fill(tgt_mask[:, None, None, :], float("-inf"))
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))           # softmax numerators: stored; their sum: fp32
        o = r((r(e) @ v) / e.sum(dim=-1, keepdim=True)).transpose(1, 2).reshape(B, T, H)
        a = F.linear(o, r(t("self_attn.out_proj.weight")), t("self_attn.out_proj.bias"))
        x = r(F.layer_norm(x + a, (H,), t("norm1.weight"), t("norm1.bias"), 1e-5))
        y = x.transpose(1, 2)
        if cfg.decoder_depthwise_conv:
            y = r(F.conv1d(y, t("conv1.0.weight"), t("conv1.0.bias"), padding="same", groups=H))
            y = r(torch.relu(F.conv1d(y, r(t("conv1.1.weight")), t("conv1.1.bias"))))
            G, bg, W2, b2 = t("conv2.0.weight").double(), t("conv2.0.bias").double(), t("conv2.1.weight").double(), t("conv2.1.bias").double()
            Fch, gs = G.shape[0], G.shape[1]
            W2g = W2[:, :, 0].reshape(H, H, gs)                    # [o][group][i]
            Wf = torch.einsum("ogi,gij->ogj", W2g, G[:, :, 0].reshape(H, gs, gs)).reshape(H, Fch)
            bf = b2 + W2[:, :, 0] @ bg
            y = F.conv1d(y, r(Wf.float())[:, :, None], bf.float())
        else:
            y = r(torch.relu(F.conv1d(y, r(t("conv1.weight")), t("conv1.bias"), padding="same")))
            y = F.conv1d(y, r(t("conv2.weight")), t("conv2.bias"), padding="same")
        x = r(F.layer_norm(x + y.transpose(1, 2), (H,), t("norm2.weight"), t("norm2.bias"), 1e-5))
    return F.linear(x, r(O._t(sd, "linear.weight")), O._t(sd, "linear.bias"))
