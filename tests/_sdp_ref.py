"""CPU restatement of the stochastic duration predictor at inference, written from its definition (a StochasticDurationPredictor
with reverse=True behind StochasticDurationPredictorWrapper): text conditioning through a dilated depth-separable conv stack, the
reversed flow loop of rational-quadratic spline ConvFlows, the closing element-wise affine, and the durations rule of the
stochastic model.  torch on the CPU, in the dtype of the weights handed in (float64 for the truth, float32 for an equal-precision
yardstick).  Nothing here is used by the product path."""
import math

import numpy as np
import torch
import torch.nn.functional as F

PREFIX = "variance_adaptor.duration_predictor."
NUM_BINS = 10
TAIL = 5.0
MIN_W = MIN_H = MIN_D = 1e-3


def sdp_weights(sd, dtype=torch.float64):
    """The sdp.* tensors of a full state_dict (or of one already relative to the duration predictor), as torch tensors of dtype."""
    out = {}
    for k, v in sd.items():
        if k.startswith(PREFIX):
            k = k[len(PREFIX):]
        if k.startswith("sdp."):
            out[k] = torch.as_tensor(np.asarray(v)).to(dtype)
    return out


def n_flows(w):
    return max(int(k.split(".")[2]) for k in w if k.startswith("sdp.flows."))


def layer_norm(x, gamma, beta, eps=1e-5):  # over the channel axis of (B, C, L)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma[None, :, None] + beta[None, :, None]


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dds(w, p, x, m, g=None):
    """x (B, C, L), m (B, 1, L) of x's dtype"""
    if g is not None:
        x = x + g
    C = x.shape[1]
    for i in range(3):
        k = w[f"{p}.convs_sep.{i}.weight"].shape[-1]
        dil = k ** i
        y = F.conv1d(x * m, w[f"{p}.convs_sep.{i}.weight"], w[f"{p}.convs_sep.{i}.bias"], padding=(k * dil - dil) // 2,
                     dilation=dil, groups=C)
        y = gelu(layer_norm(y, w[f"{p}.norms_1.{i}.gamma"], w[f"{p}.norms_1.{i}.beta"]))
        y = F.conv1d(y, w[f"{p}.convs_1x1.{i}.weight"], w[f"{p}.convs_1x1.{i}.bias"])
        y = gelu(layer_norm(y, w[f"{p}.norms_2.{i}.gamma"], w[f"{p}.norms_2.{i}.beta"]))
        x = x + y
    return x * m


def spline_inverse(x, h, sqrt_f, return_details=False):
    """x (...), h (..., 29): the inverse of the unconstrained rational-quadratic spline with linear tails, tail bound 5, 10 bins.
    return_details: also the discriminant (1 outside the bound) and the bin each value fell into (-1 outside the bound)."""
    dt = x.dtype
    inside = (x >= -TAIL) & (x <= TAIL)
    xs = torch.where(inside, x, torch.zeros_like(x))  # evaluated everywhere, selected below
    uw, uh, ud = h[..., :NUM_BINS] / sqrt_f, h[..., NUM_BINS:2 * NUM_BINS] / sqrt_f, h[..., 2 * NUM_BINS:]
    edge = torch.full(ud.shape[:-1] + (1,), math.log(math.exp(1.0 - MIN_D) - 1.0), dtype=dt)
    ud = torch.cat([edge, ud, edge], -1)

    def knots(u, min_size):
        s = min_size + (1.0 - min_size * NUM_BINS) * torch.softmax(u, -1)
        c = torch.cumsum(s, -1)
        c = torch.cat([torch.zeros_like(c[..., :1]), c], -1) * (2 * TAIL) - TAIL
        c[..., 0] = -TAIL
        c[..., -1] = TAIL
        return c, c[..., 1:] - c[..., :-1]

    cw, widths = knots(uw, MIN_W)
    ch, heights = knots(uh, MIN_H)
    deriv = MIN_D + F.softplus(ud)
    search = ch.clone()
    search[..., -1] += 1e-6
    idx = ((xs[..., None] >= search).sum(-1) - 1).clamp(0, NUM_BINS - 1)[..., None]
    pick = lambda t: t.gather(-1, idx)[..., 0]
    icw, ibw, ich, ih = pick(cw), pick(widths), pick(ch), pick(heights)
    delta = ih / ibw
    d0, d1 = pick(deriv), pick(deriv[..., 1:])
    t = xs - ich
    s = d0 + d1 - 2 * delta
    a = t * s + ih * (delta - d0)
    b = ih * d0 - t * s
    c = -delta * t
    disc = b * b - 4 * a * c
    root = (2 * c) / (-b - torch.sqrt(disc.clamp(min=0)))
    out = torch.where(inside, root * ibw + icw, x)
    if return_details:
        return out, torch.where(inside, disc, torch.ones_like(disc)), torch.where(inside, idx[..., 0], torch.full_like(idx[..., 0], -1))
    return out


def conv_flow_reverse(w, p, z, m, g):
    x0, x1 = z[:, :1], z[:, 1:]
    h = F.conv1d(x0, w[f"{p}.pre.weight"], w[f"{p}.pre.bias"])
    h = dds(w, f"{p}.convs", h, m, g=g)
    h = F.conv1d(h, w[f"{p}.proj.weight"], w[f"{p}.proj.bias"]) * m  # (B, 29, L)
    sqrt_f = math.sqrt(w[f"{p}.pre.weight"].shape[0])
    x1n = spline_inverse(x1[:, 0], h.transpose(1, 2), sqrt_f)
    return torch.cat([x0, x1n[:, None]], 1) * m


def sdp_logw(w, x, pad, noise):
    """w: sdp_weights(...); x (B, L, H); pad (B, L) bool, True = pad; noise (B, 2, L) already scaled.  -> logw (B, L), 0 at pads."""
    dt = next(iter(w.values())).dtype
    x = torch.as_tensor(x).to(dt).transpose(1, 2)
    pad = torch.as_tensor(pad).bool()
    m = (~pad)[:, None].to(dt)
    z = torch.as_tensor(noise).to(dt)
    g = F.conv1d(x, w["sdp.pre.weight"], w["sdp.pre.bias"])
    g = dds(w, "sdp.convs", g, m)
    g = F.conv1d(g, w["sdp.proj.weight"], w["sdp.proj.bias"]) * m
    n = n_flows(w)
    for j in list(range(n, 1, -1)) + [0]:  # CF_n .. CF_2, then the element-wise affine; CF_1 never runs
        z = torch.flip(z, [1])
        if j == 0:
            z = (z - w["sdp.flows.0.translation"]) * torch.exp(-w["sdp.flows.0.log_scale"]) * m
        else:
            z = conv_flow_reverse(w, f"sdp.flows.{j}", z, m, g)
    return z[:, 0].masked_fill(pad, 0)


def durations_stochastic(logw, pad=None, forced=None):
    """The stochastic model's rounding, as written in float32, then the zero-duration guard: -> (durations int32, guard (B) bool)"""
    logw = torch.as_tensor(logw).to(torch.float32)
    B, L = logw.shape
    pad = torch.zeros(B, L, dtype=torch.bool) if pad is None else torch.as_tensor(pad).bool()
    guard = torch.zeros(B, dtype=torch.bool)
    if forced is not None:
        return torch.as_tensor(forced).to(torch.int32).clamp(min=0), guard
    d = torch.ceil(torch.exp(logw + 1e-9)).masked_fill(logw == 0, 0)
    d = torch.clamp(d, min=0).to(torch.int32)
    for b in range(B):
        v = ~pad[b]
        if int(d[b][v].sum()) <= int(v.sum()) // 2:
            d[b][v] = 1
            guard[b] = True
    return d, guard


# ---- the frozen recipe of the module fixtures (tests/golden/sdp/module_n*.npz; tools/gen_golden_sdp.py) -------------------------
MODULE_B, MODULE_L, MODULE_LENGTHS = 3, 150, (150, 1, 75)


def module_config(n, hidden=256):
    """The smallest Fs2Config whose state_dict holds a stochastic duration predictor of n flows on `hidden` encoder channels."""
    from lightningfastspeech2_amd.config import Fs2Config
    return Fs2Config(n_phones=20, encoder_hidden=hidden, decoder_hidden=hidden, encoder_layers=1, decoder_layers=1,
                     encoder_kernel_sizes=[3], decoder_kernel_sizes=[3], encoder_conv_filter_size=hidden,
                     decoder_conv_filter_size=hidden, encoder_depthwise_conv=False, decoder_depthwise_conv=False, variances=[],
                     variance_levels=[], variance_transforms=[], variance_nlayers=[], variance_kernel_size=[],
                     variance_depthwise_conv=False, duration_nlayers=n, duration_kernel_size=3, duration_filter_size=256,
                     duration_depthwise_conv=False, duration_stochastic=True)


def module_inputs(seed, B=MODULE_B, L=MODULE_L, lengths=MODULE_LENGTHS, hidden=256):
    """x (B, L, hidden) float32 ~ N(0, 1) (an encoder output's scale), pad (B, L) bool from the lengths"""
    x = np.random.RandomState(seed).standard_normal((B, L, hidden)).astype(np.float32)
    pad = np.arange(L)[None, :] >= np.asarray(lengths)[:, None]
    return x, pad


def sdp_state_dict(cfg, seed):
    """the sdp.* part of the synthetic state_dict, names relative to the duration predictor, float32 numpy"""
    from lightningfastspeech2_amd.weights import synth_state_dict
    return {k[len(PREFIX):]: v for k, v in synth_state_dict(cfg, seed).items() if k.startswith(PREFIX + "sdp.")}


def digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        if isinstance(a, dict):
            for k in a:
                h.update(k.encode())
                h.update(np.ascontiguousarray(a[k]).tobytes())
        else:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
