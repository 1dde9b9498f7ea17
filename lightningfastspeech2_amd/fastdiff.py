"""Host mirror of the reference's FastDiff vocoder at inference (litfass/third_party/fastdiff/FastDiff.py, module/modules.py,
module/util.py): what ``SpeechGenerator(fastdiff=True)`` calls as ``model.fastdiff_model.inference(mel, N=4)``
(synthesis/generator.py:48-57, 166-168).  ``FastDiff.denoise`` is one ``FastDiff.forward(x, c, ts)`` (the eps network),
``FastDiff.inference`` the reverse sampler (util.py:158-237, ddim off) with the peak normalisation of FastDiff.py:193.

All arithmetic runs in libfs2_hip.so through the ``fs2_fd_*`` C ABI (csrc/fastdiff.hip); torch is used for device memory, streams
and the CPU generator's noise.  There is no CPU fallback.

Out of scope: training (``forward`` without ``ts``, ``theta_timestep_loss``), ddim, N = 200 / 1000, other architectures, the
FastDiff variance adaptor / speaker generator, and the ``fastdiff_var`` output of the mel forward (fastspeech2.py:733-736: the
reference adds it to the mel before vocoding; a caller adds it to ``mel`` themselves)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .hifigan import fold_weight_norm

_RESIDUAL_IDX = (1, 3, 6, 8, 11, 13)  # the Conv1d entries of KernelPredictor.residual_conv (modules.py:297-313)

# FastDiff.inference's tabulated schedules (FastDiff.py:163-172)
_BETAS = {
    8: [6.689325005027058e-07, 1.0033881153503899e-05, 0.00015496854030061513, 0.002387222135439515, 0.035597629845142365,
        0.3681158423423767, 0.4735414385795593, 0.5],
    6: [1.7838445955931093e-06, 2.7984189728158526e-05, 0.00043231004383414984, 0.006634317338466644, 0.09357017278671265,
        0.6000000238418579],
    4: [3.2176e-04, 2.5743e-03, 2.5376e-02, 7.0414e-01],
    3: [9.0000e-05, 9.0000e-03, 6.0000e-01],
}


@dataclass
class FastDiffConfig:
    """The reference's constructor arguments (FastDiff.py:14-32)."""
    audio_channels: int = 1
    inner_channels: int = 32
    cond_channels: int = 80
    upsample_ratios: List[int] = field(default_factory=lambda: [8, 8, 4])
    lvc_layers_each_block: int = 4
    lvc_kernel_size: int = 3
    kpnet_hidden_channels: int = 64
    kpnet_conv_size: int = 3
    dropout: float = 0.0
    diffusion_step_embed_dim_in: int = 128
    diffusion_step_embed_dim_mid: int = 512
    diffusion_step_embed_dim_out: int = 512
    use_weight_norm: bool = True
    beta_0: float = 1e-6
    beta_T: float = 0.01
    T: int = 1000

    @property
    def hop(self) -> int:
        return int(np.prod(self.upsample_ratios))

    @classmethod
    def from_hparams(cls, hparams) -> "FastDiffConfig":
        """The ``--fastdiff_*`` flags (FastDiff.add_model_specific_args): a dict or a namespace."""
        get = hparams.get if isinstance(hparams, dict) else lambda k, d=None: getattr(hparams, k, d)
        kw = {}
        for f in cls.__dataclass_fields__:
            v = get("fastdiff_" + f, None)
            if v is not None:
                kw[f] = list(v) if f == "upsample_ratios" else v
        return cls(**kw)

    def supported(self) -> bool:
        """What the kernels cover (fs2_fd_supported): the reference's default architecture and training schedule."""
        r = (C.c_int32 * len(self.upsample_ratios))(*self.upsample_ratios)
        return bool(_lib.load().fs2_fd_supported(*self._c_args(r))) and self._schedule_is_default()

    def _schedule_is_default(self) -> bool:
        return self.audio_channels == 1 and self.T == 1000 and self.beta_0 == 1e-6 and self.beta_T == 0.01

    def _c_args(self, ratios):
        return (self.inner_channels, self.cond_channels, ratios, len(self.upsample_ratios), self.lvc_layers_each_block,
                self.lvc_kernel_size, self.kpnet_hidden_channels, self.kpnet_conv_size, self.diffusion_step_embed_dim_in,
                self.diffusion_step_embed_dim_mid, self.diffusion_step_embed_dim_out)


def state_dict_spec(cfg: FastDiffConfig) -> Dict[str, tuple]:
    """FastDiff.state_dict() names / shapes after remove_weight_norm (modules in their registration order)."""
    ic, cc, hid = cfg.inner_channels, cfg.cond_channels, cfg.kpnet_hidden_channels
    L, k = cfg.lvc_layers_each_block, cfg.lvc_kernel_size
    s: Dict[str, tuple] = {}

    def conv(name, n, cin, ks):
        s[name + ".weight"] = (n, cin, ks)
        s[name + ".bias"] = (n,)

    def linear(name, n, cin):
        s[name + ".weight"] = (n, cin)
        s[name + ".bias"] = (n,)

    conv("first_audio_conv", ic, cfg.audio_channels, 7)
    nb = len(cfg.upsample_ratios)
    for n, r in enumerate(cfg.upsample_ratios):
        p = f"lvc_blocks.{n}"
        for i in range(L):
            conv(p + f".convs.{i}", ic, ic, k)
        s[p + ".upsample.weight"] = (ic, ic, 2 * r)  # ConvTranspose1d: (in, out, k); never weight-normed
        s[p + ".upsample.bias"] = (ic,)
        kp = p + ".kernel_predictor"
        conv(kp + ".input_conv.0", hid, cc, 5)
        for i in _RESIDUAL_IDX:
            conv(kp + f".residual_conv.{i}", hid, hid, cfg.kpnet_conv_size)
        conv(kp + ".kernel_conv", ic * 2 * ic * k * L, hid, cfg.kpnet_conv_size)
        conv(kp + ".bias_conv", 2 * ic * L, hid, cfg.kpnet_conv_size)
        linear(p + ".fc_t", cc, cfg.diffusion_step_embed_dim_out)
    for n in range(nb):
        d = f"downsample.{n}"
        conv(d + ".residual_dense", ic, ic, 1)
        for i in range(3):
            conv(d + f".conv.{i}", ic, ic, 3)
    linear("fc_t1", cfg.diffusion_step_embed_dim_mid, cfg.diffusion_step_embed_dim_in)
    linear("fc_t2", cfg.diffusion_step_embed_dim_out, cfg.diffusion_step_embed_dim_mid)
    conv("final_conv.0", cfg.audio_channels, ic, 7)
    return s


def synth_state_dict(cfg: FastDiffConfig, seed: int = 0) -> Dict[str, np.ndarray]:
    """Random weights (no FastDiff checkpoint ships with the reference): N(0, 1 / fan_in) weights and small biases so activations stay
    O(1); ``kernel_conv`` scaled so that a predicted LVC kernel has variance about 1 / 96 (the LVC's own fan-in: 32 channels x 3 taps)
    and ``final_conv`` by 0.2 so that eps is O(1).  numpy RandomState, names drawn in sorted order: identical on every host."""
    rs = np.random.RandomState(seed)
    spec = state_dict_spec(cfg)
    lvc_fan = cfg.inner_channels * cfg.lvc_kernel_size
    sd = {}
    for name in sorted(spec):
        shape = spec[name]
        if name.endswith(".bias"):
            sd[name] = (0.05 * rs.standard_normal(shape)).astype(np.float32)
            continue
        if ".upsample." in name:
            cin, _, k = shape
            r = k // 2
            std = (r / (cin * k)) ** 0.5
        else:
            std = (1.0 / np.prod(shape[1:])) ** 0.5
        if ".kernel_conv." in name:
            std *= (1.0 / lvc_fan) ** 0.5
        if name.startswith("final_conv"):
            std *= 0.2
        sd[name] = (rs.standard_normal(shape) * std).astype(np.float32)
    return sd


def _sqrt_rounded(t: torch.Tensor) -> torch.Tensor:
    """The correctly rounded float32 square root, element by element: the float64 square root (IEEE, through math.sqrt) rounded once to
    float32 is the correctly rounded float32 root (53 >= 2 x 24 + 2 significand bits)."""
    return torch.tensor([math.sqrt(v) for v in t.tolist()], dtype=torch.float64).to(torch.float32)


def inference_schedule(N: int, sqrt=_sqrt_rounded) -> Dict[str, torch.Tensor]:
    """``beta``, ``alpha`` (the cumulative sqrt(prod(1 - beta))), ``sigma`` and the fractional ``steps`` of FastDiff.inference(N),
    float32 with the reference's own tensor operations in its order (FastDiff.py:88-89, util.py:187-204, 276-316), except that the
    three square roots are correctly rounded, as the engine's are (fs2_fd_schedule: the same in scalar float arithmetic with sqrtf);
    the two agree bit for bit for every N, on every host.

    ``sqrt=torch.sqrt`` gives what the reference computes ON THIS HOST.  torch's CPU sqrt is not correctly rounded, and how far off it
    is depends on the CPU's vector path: measured, one x86 host rounds 4 of the 1000 training alphas and one near-tie the other way,
    another 218 of the 1000 and a fifth of all small inputs, which moves the fractional steps of every N by up to 1e-2.  On the host
    that recorded tests/golden/fastdiff/ the reference's schedules for N = 3, 4 and 8 ARE the correctly rounded ones, bit for bit;
    for N = 6 the cumulative alpha of step 4 is a near-tie (0.948683411...) that its torch rounded down: the engine's alpha[4] is one
    float32 ulp above the recorded one, which moves that step's 144.46 down by six float32 ulps (9.2e-5); every other entry agrees
    bit for bit.  All of this is pinned by tests/test_fastdiff_cpu.py; the N = 6 waveform moves by 2.4e-7 at most."""
    if N not in _BETAS:
        raise ValueError("Reverse step should be 3, 4, 6 or 8 (200 and 1000 are not supported).")
    train = torch.linspace(1e-6, 0.01, 1000)
    alpha_t = 1 - train
    for t in range(1, 1000):
        alpha_t[t] *= alpha_t[t - 1]
    alpha_t = sqrt(alpha_t)
    beta = torch.FloatTensor(_BETAS[N])
    alpha = 1 - beta
    sigma = beta + 0
    for n in range(1, N):
        alpha[n] *= alpha[n - 1]
        sigma[n] *= (1 - alpha[n - 1]) / (1 - alpha[n])
    alpha, sigma = sqrt(alpha), sqrt(sigma)
    steps = []
    for n in range(N):
        a = alpha[n]
        if a < alpha_t[-1]:
            steps.append(999)
        elif a > alpha_t[0]:
            steps.append(0)
        else:
            for t in range(999):
                if alpha_t[t + 1] <= a <= alpha_t[t]:
                    d = alpha_t[t] - a
                    d = d / (alpha_t[t] - alpha_t[t + 1])
                    steps.append(t + d.item())
                    break
    return {"beta": beta, "alpha": alpha, "sigma": sigma, "steps": torch.FloatTensor(steps)}


def draw_noise(lengths: Sequence[int], N: int = 4, hop: int = 256, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The reference's draws in the reference's order on the CPU generator: utterance after utterance (generator.py:163-168), per
    utterance ``x_T`` first, then one ``(1, 1, S_i)`` draw per reverse step with n > 0 (util.py:211, 231).  Returns (N, B, max S)
    float32 with zeros past an utterance's samples: [0] is x_T, [j] the draw of step n = N - j."""
    lengths = [int(v) for v in lengths]
    S = max(lengths) * hop
    out = torch.zeros(N, len(lengths), S)
    for b, frames in enumerate(lengths):
        for j in range(N):
            out[j, b, :frames * hop] = torch.normal(0, 1, size=(1, 1, frames * hop), generator=generator).view(-1)
    return out


_PRECISIONS = {"bf16": _lib.FS2_BF16, "fp32": _lib.FS2_F32}
_TORCH_DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


class FastDiff(_lib.Handle):
    """Device-resident FastDiff.  ``state_dict``: the reference's names, checkpoint form (weight_g / weight_v) or plain.
    ``precision``: "fp32" (parity mode) or "bf16" (weights, predicted kernels and the streams between launches in bf16; the
    diffusion state, noise, eps, sampler and gate arithmetic stay fp32)."""
    _prefix = "fs2_fd"
    _label = "fastdiff "
    _load_what = "load_weight {}"

    def __init__(self, cfg: FastDiffConfig, state_dict, precision: str = "bf16", device="cuda:0"):
        self.cfg, self.device = cfg, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FastDiff runs on an MI355X only (no CPU fallback)")
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
        if not cfg._schedule_is_default():
            raise ValueError("only the reference's training schedule (beta 1e-6 .. 0.01, T = 1000, one audio channel) is supported")
        _lib.Handle.__init__(self)
        self.precision, self.dtype = precision, _PRECISIONS[precision]
        ratios = (C.c_int32 * len(cfg.upsample_ratios))(*cfg.upsample_ratios)
        with torch.cuda.device(self.device):
            st = self.lib.fs2_fd_create(_lib.FS2_ABI_VERSION, self.dtype, *cfg._c_args(ratios), C.byref(self.handle))
            try:
                self._check(st, "create")
                sd = fold_weight_norm(state_dict)
                spec = state_dict_spec(cfg)
                missing = [k for k in spec if k not in sd]
                if missing:
                    raise KeyError(f"FastDiff weights missing: {missing[:4]}{'...' if len(missing) > 4 else ''}")
                self.load_weights(spec, sd)
            except Exception:
                self.close()
                raise
        self.hop = int(self.lib.fs2_fd_hop(self.handle))

    @property
    def tile_rows(self) -> int:
        return int(self.lib.fs2_fd_tile_rows(self.handle))

    def launches(self, N: int = 0) -> int:
        """kernel launches per utterance chunk of ``inference(N=N)``; N = 0: of one ``denoise``"""
        return int(self.lib.fs2_fd_launches(self.handle, N))

    def set_chunk(self, max_utterances: int = 0):
        """Walk a batch in chunks of at most this many utterances (0: as many as fit the default workspace cap)."""
        self._check(self.lib.fs2_fd_set_chunk(self.handle, max_utterances), "set_chunk")

    def workspace_bytes(self, B: int, T: int) -> int:
        n = C.c_size_t()
        self._check(self.lib.fs2_fd_workspace_bytes(self.handle, B, T, C.byref(n)), "workspace_bytes")
        return n.value

    def _inputs(self, mel, lengths):
        mel = mel.to(self.device, torch.float32).contiguous()
        if mel.dim() != 3 or mel.shape[2] != self.cfg.cond_channels:
            raise ValueError(f"mel must be (B, T, {self.cfg.cond_channels})")
        ld = None if lengths is None else torch.as_tensor(lengths).to(self.device, torch.int32).contiguous()
        if ld is not None and ld.numel() != mel.shape[0]:
            raise ValueError("lengths must be (B,)")
        return mel, ld

    def denoise(self, x: torch.Tensor, mel: torch.Tensor, lengths=None, step: float = 0.0, out: Optional[torch.Tensor] = None):
        """One eps evaluation: x (B, T*hop) fp32, mel (B, T, 80), lengths (B,) frames or None, step the fractional diffusion step
        -> eps (B, T*hop) fp32 (zeros past an utterance's samples unless ``out`` is given: those are left untouched)."""
        mel, ld = self._inputs(mel, lengths)
        B, T, _ = mel.shape
        x = x.to(self.device, torch.float32).contiguous()
        if tuple(x.shape) != (B, T * self.hop):
            raise ValueError(f"x must be ({B}, {T * self.hop})")
        eps = out if out is not None else torch.zeros(B, T * self.hop, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(self.workspace_bytes(B, T))
            self._check(self.lib.fs2_fd_denoise(self.handle, x, mel, ld, float(step), eps, ws, ws.numel(), B, T,
                                                torch.cuda.current_stream(self.device)), "denoise")
        return eps

    def _sample(self, mel, ld, N, noise, wav):
        B, T, _ = mel.shape
        if noise is None:
            frames = [T] * B if ld is None else ld.cpu().tolist()  # the CPU generator's draws need the lengths on the host
            noise = draw_noise(frames, N, self.hop)
            if noise.shape[2] < T * self.hop:
                noise = torch.nn.functional.pad(noise, (0, T * self.hop - noise.shape[2]))
        noise = noise.to(self.device, torch.float32).contiguous()
        if tuple(noise.shape) != (N, B, T * self.hop):
            raise ValueError(f"noise must be ({N}, {B}, {T * self.hop})")
        with torch.cuda.device(self.device):
            ws = self._workspace(self.workspace_bytes(B, T))
            self._check(self.lib.fs2_fd_sample(self.handle, mel, ld, noise, N, wav, ws, ws.numel(), B, T,
                                               torch.cuda.current_stream(self.device)), "sample")
        return wav

    def inference(self, mel: torch.Tensor, lengths=None, N: int = 4, noise: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """FastDiff.inference for a padded batch: mel (B, T, 80) -> wav (B, T*hop) fp32, every utterance peak-normalised over its own
        samples (zeros past them unless ``out`` is given: those are left untouched).  ``noise``: (N, B, T*hop) as ``draw_noise``
        lays it out; None draws it from torch's CPU generator exactly as the reference would, utterance after utterance."""
        mel, ld = self._inputs(mel, lengths)
        B, T, _ = mel.shape
        wav = out if out is not None else torch.zeros(B, T * self.hop, dtype=torch.float32, device=self.device)
        return self._sample(mel, ld, N, noise, wav)

    def synthesize_packed(self, mel: torch.Tensor, lengths=None, dtype: str = "float32", out: Optional[torch.Tensor] = None, N: int = 4,
                          noise: Optional[torch.Tensor] = None):
        """The signature ``SpeechGenerator`` uses (``HifiGan.synthesize_packed``): ``(packed, offsets)`` device tensors, utterance b's
        samples are ``packed[offsets[b]:offsets[b+1]]``.  The samples are the float32 waveform itself, UNQUANTISED: the reference
        hands FastDiff's tensor to int16_samples_to_float32, which passes float32 through (generator.py:24-33, 166-168)."""
        if dtype != "float32":
            raise ValueError("FastDiff's samples are float32 (the reference does not quantise them)")
        mel, ld = self._inputs(mel, lengths)
        B, T, _ = mel.shape
        wav = self._sample(mel, ld, N, noise, torch.empty(B, T * self.hop, dtype=torch.float32, device=self.device))
        if ld is None:
            ld = torch.full((B,), T, dtype=torch.int32, device=self.device)
        offsets = torch.zeros(B + 1, dtype=torch.int64, device=self.device)
        offsets[1:] = torch.cumsum(ld.to(torch.int64) * self.hop, 0)
        keep = torch.arange(T * self.hop, device=self.device)[None, :] < (ld.to(torch.int64) * self.hop)[:, None]
        packed = wav[keep]  # the utterances' own samples, one after the other
        if out is not None:
            out[:packed.numel()] = packed
            packed = out
        return packed, offsets

    # ---- the pieces the tests take apart ----
    def predict_kernels(self, block: int, mel: torch.Tensor, lengths=None, step: float = 0.0):
        """Kernel predictor of LVC block ``block``: ``(kernels (B, T, 24576) in the LVC launch's order, bias (B, T, 256))`` in the
        engine's storage dtype; ``kernel_index`` maps the reference's (layer, in, out, k) to a position."""
        mel, ld = self._inputs(mel, lengths)
        B, T, _ = mel.shape
        td = _TORCH_DTYPES[self.precision]
        K = torch.zeros(B, T, 24576, dtype=td, device=self.device)
        kb = torch.zeros(B, T, 256, dtype=td, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(self.workspace_bytes(B, T))
            self._check(self.lib.fs2_fd_predict_kernels(self.handle, block, mel, ld, float(step), K, kb, ws, ws.numel(), B, T,
                                                        torch.cuda.current_stream(self.device)), "predict_kernels")
        return K, kb

    def dblock(self, block: int, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """DiffusionDBlock ``block`` (factors 4, 8, 8): x (B, S, 32) in the storage dtype -> (B, S / f, 32)."""
        f, per_frame = (4, 8, 8)[block], (256, 64, 8)[block]
        B, S, _ = x.shape
        T = S // per_frame
        x = x.to(self.device, _TORCH_DTYPES[self.precision]).contiguous()
        ld = None if lengths is None else torch.as_tensor(lengths).to(self.device, torch.int32).contiguous()
        out = torch.zeros(B, S // f, 32, dtype=x.dtype, device=self.device)
        tmp = torch.empty(3, B, S // f, 32, dtype=x.dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.fs2_op_fd_dblock(self.handle, block, x, out, tmp, ld, B, T, torch.cuda.current_stream(self.device)),
                        "op_fd_dblock")
        return out


def kernel_index(precision: str = "fp32") -> np.ndarray:
    """(4, 32, 64, 3) int64: the position of the reference's kernels[layer, in, out, k] inside a frame's 24576 predicted values."""
    lib, dt = _lib.load(), _PRECISIONS[precision]
    idx = np.empty((4, 32, 64, 3), np.int64)
    for l in range(4):
        for c in range(32):
            for o in range(64):
                for k in range(3):
                    idx[l, c, o, k] = lib.fs2_fd_kernel_index(dt, l, c, o, k)
    return idx


def lvc(y, kernels, bias, x, add, lengths, hop: int, layer: int, precision: str = "fp32") -> torch.Tensor:
    """fs2_op_lvc: y, x, add (B, T*hop, 32), kernels (B, T, 24576) in the launch's order, bias (B, T, 256), all device tensors of
    the precision's dtype -> x + sigmoid(o[:, :32]) * tanh(o[:, 32:]) (+ add)."""
    B, S, _ = x.shape
    out = torch.zeros_like(x)
    ld = None if lengths is None else torch.as_tensor(lengths).to(x.device, torch.int32).contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().fs2_op_lvc(_PRECISIONS[precision], hop, layer, y.contiguous(), kernels.contiguous(), bias.contiguous(),
                                          x.contiguous(), None if add is None else add.contiguous(), out, ld, B, S // hop,
                                          torch.cuda.current_stream(x.device)), what="op_lvc")
    return out
