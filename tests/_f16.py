"""Helpers of the FS2_F16 / precision="mixed16" tests.

(a) The storage rule on the host (`store`, `rnd16`, `f16_bits`) - tests/_gpu.py's operator wrappers upload through it - and the
    edge-value vector the conversion tests share.  Nothing here needs a GPU.
(b) `decoder_16bit`: a plain-torch CPU model of a decoder that STORES its tensors in a 16-bit type - the yardstick the end-to-end
    tests hold the engine's decoder to.  It restates what the engine rounds, nothing else: the matrix weights, the decoder input,
    qkv, the softmax numerators, the normalised attention output, both LayerNorm outputs, the depth-wise conv output and the
    post-ReLU FFN tensor go through the storage type; accumulation, softmax statistics, LayerNorm, biases and the depth-wise
    weights stay fp32.  Parameterised by torch.bfloat16 / torch.float16, so the same code models the "mixed3" and the "mixed16" back.
"""
import math

import torch
import torch.nn.functional as F

F16_MAX = 65504.0


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
