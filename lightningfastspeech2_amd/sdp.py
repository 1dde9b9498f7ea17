"""The stochastic duration predictor at inference (``duration_stochastic=True``) as a module of its own: ``fs2_sdp_*`` of
include/fs2.h (csrc/sdp.hip).  It plays the role of the reference's ``StochasticDurationPredictorWrapper(...)(x, mask,
inference=True)`` (litfass/fastspeech2/model.py:463-479) with the noise handed in, so a forward is reproducible: the reference
draws ``torch.randn(B, 2, L)`` on the CPU generator (sdp.py:335-338) and ``draw_noise`` does the same.

All arithmetic happens in libfs2_hip.so; torch is used for device memory and streams only.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from .weights import SDP_PREFIX

_DTYPES = {torch.float32: _lib.FS2_F32, torch.bfloat16: _lib.FS2_BF16, torch.float16: _lib.FS2_F16}


def draw_noise(B: int, L: int, noise_scale: float = 1.0) -> torch.Tensor:
    """The reference's draw: one ``torch.randn(B, 2, L)`` on the CPU default generator, times ``noise_scale`` (its ``sigma``)."""
    return torch.randn(B, 2, L) * noise_scale


def supported(in_channels: int, filter_size: int, kernel_size: int, n_flows: int) -> bool:
    return bool(_lib.load().fs2_sdp_supported(in_channels, filter_size, kernel_size, n_flows))


class StochasticDurationPredictor(_lib.Handle):
    """One ``fs2_sdp`` handle.  ``state_dict``: the reference's names, either full (``variance_adaptor.duration_predictor.sdp.*``)
    or relative to the duration predictor (``sdp.*``); the training-only tensors may be present (they are checked and dropped) or
    absent."""
    _prefix = "fs2_sdp"
    _label = "sdp "

    def __init__(self, in_channels: int, filter_size: int, kernel_size: int, n_flows: int, state_dict, device="cuda:0"):
        _lib.Handle.__init__(self)
        self.device = torch.device(device)
        self.in_channels, self.n_flows = in_channels, n_flows
        st = self.lib.fs2_sdp_create(_lib.FS2_ABI_VERSION, in_channels, filter_size, kernel_size, n_flows, C.byref(self.handle))
        try:
            self._check(st, "create")
            # (a tensor present under both its full and its relative name is loaded once, with the value that comes later in
            #  state_dict: what two loads in order left in the handle)
            sd = {(k[len(SDP_PREFIX):] if k.startswith(SDP_PREFIX) else k): v for k, v in state_dict.items()}
            with torch.cuda.device(self.device):
                self.load_weights([k for k in sd if k.startswith("sdp.")], sd)
        except Exception:
            self.close()
            raise

    @property
    def tile_rows(self) -> int:
        return int(self.lib.fs2_sdp_tile_rows(self.handle))

    @property
    def launches(self) -> int:
        """kernel launches of one forward: the conditioning, one per ConvFlow that runs (a lone row launch for one flow)"""
        return int(self.lib.fs2_sdp_launches(self.handle))

    def workspace_bytes(self, B: int, L: int) -> int:
        n = C.c_size_t()
        self._check(self.lib.fs2_sdp_workspace_bytes(self.handle, B, L, C.byref(n)), "workspace_bytes")
        return n.value

    def forward(self, x: torch.Tensor, pad_mask: torch.Tensor, noise: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x (B, L, H) fp32 / bf16 / fp16, pad_mask (B, L) bool (True = pad), noise (B, 2, L) already scaled -> logw (B, L) fp32"""
        if x.dim() != 3 or x.shape[2] != self.in_channels or x.dtype not in _DTYPES:
            raise ValueError(f"x must be (B, L, {self.in_channels}) in float32, bfloat16 or float16")
        B, L, _ = x.shape
        if tuple(pad_mask.shape) != (B, L) or tuple(noise.shape) != (B, 2, L):
            raise ValueError(f"pad_mask must be ({B}, {L}) and noise ({B}, 2, {L})")
        x = x.to(self.device).contiguous()
        pad = pad_mask.to(self.device, dtype=torch.uint8).contiguous()
        noise = noise.to(self.device, dtype=torch.float32).contiguous()
        logw = out if out is not None else torch.empty(B, L, dtype=torch.float32, device=self.device)
        ws = self._workspace(self.workspace_bytes(B, L))
        with torch.cuda.device(self.device):
            st = self.lib.fs2_sdp_forward(self.handle, _DTYPES[x.dtype], x, pad, noise, logw, ws, ws.numel(), B, L,
                                          torch.cuda.current_stream(self.device))
        self._check(st, "forward")
        return logw

    __call__ = forward


def rq_spline_inverse(x1: torch.Tensor, h29: torch.Tensor, filter_size: int = 256) -> torch.Tensor:
    """fs2_op_rq_spline_inverse: x1 (rows) and h29 (rows, 29) fp32 device tensors -> (rows)"""
    x1, h29 = x1.contiguous().float(), h29.contiguous().float()
    if h29.shape != (x1.numel(), 29):
        raise ValueError("h29 must be (rows, 29)")
    out = torch.empty_like(x1)
    with torch.cuda.device(x1.device):
        _lib.check(_lib.load().fs2_op_rq_spline_inverse(x1, h29, filter_size, out, x1.numel(), torch.cuda.current_stream(x1.device)),
                   what="rq_spline_inverse")
    return out


def durations_stochastic(logw: torch.Tensor, src_mask: torch.Tensor, forced: Optional[torch.Tensor] = None):
    """fs2_op_durations_stochastic: logw (B, L) fp32, src_mask (B, L) bool -> dict(dur, cum (B, L) int32; totals, guard (B) int32)"""
    B, L = logw.shape
    dev = logw.device
    logw = logw.contiguous().float()
    mask = src_mask.to(dev, dtype=torch.uint8).contiguous()
    if forced is not None:
        forced = forced.to(dev, dtype=torch.int32).contiguous()
    res = {k: torch.empty(B, L, dtype=torch.int32, device=dev) for k in ("dur", "cum")}
    res.update({k: torch.empty(B, dtype=torch.int32, device=dev) for k in ("totals", "guard")})
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fs2_op_durations_stochastic(logw, mask, forced, res["dur"], res["cum"], res["totals"], res["guard"],
                                                           B, L, torch.cuda.current_stream(dev)), what="durations_stochastic")
    return res
