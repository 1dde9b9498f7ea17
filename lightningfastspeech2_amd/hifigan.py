"""Host mirror of the reference's HiFi-GAN vocoder wrapper.

Reference interface: ``litfass.third_party.hifigan.Synthesiser`` (third_party/hifigan/__init__.py:19-43):
``Synthesiser(device, model)`` loads ``generator_<model>.pth.tar``, removes weight norm, and
``synth(mel)`` maps ONE utterance's mel ``(T, 80)`` to int16 samples ``(1, T*256)``
(called per utterance by ``SpeechGenerator.generate_samples``, synthesis/generator.py:163-170).
The arithmetic (``Generator.forward``, third_party/hifigan/models.py:145-162) runs in
``libfs2_hip.so`` through the ``fs2_voc_*`` C ABI; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib


@dataclass
class HifiGanConfig:
    """The fields of third_party/hifigan/config.json that shape Generator.forward."""
    resblock: str = "1"
    upsample_rates: List[int] = field(default_factory=lambda: [8, 8, 2, 2])
    upsample_kernel_sizes: List[int] = field(default_factory=lambda: [16, 16, 4, 4])
    upsample_initial_channel: int = 512
    resblock_kernel_sizes: List[int] = field(default_factory=lambda: [3, 7, 11])
    resblock_dilation_sizes: List[List[int]] = field(default_factory=lambda: [[1, 3, 5], [1, 3, 5], [1, 3, 5]])
    num_mels: int = 80
    sampling_rate: int = 22050

    def __post_init__(self):
        if str(self.resblock) != "1":
            raise ValueError("only resblock type '1' (the shipped config) is implemented")
        if len(self.upsample_rates) != len(self.upsample_kernel_sizes):
            raise ValueError("upsample_rates / upsample_kernel_sizes length mismatch")
        if len(self.resblock_kernel_sizes) != len(self.resblock_dilation_sizes):
            raise ValueError("resblock_kernel_sizes / resblock_dilation_sizes length mismatch")
        for u, k in zip(self.upsample_rates, self.upsample_kernel_sizes):
            if (k - u) % 2 or k - 2 * ((k - u) // 2) != u:
                raise ValueError("ConvTranspose1d kernel - 2*padding must equal the stride (models.py:131-136)")
        if (self.upsample_initial_channel >> len(self.upsample_rates)) % 32:
            raise ValueError("the last stage must keep a multiple of 32 channels")

    @property
    def hop(self) -> int:
        return int(np.prod(self.upsample_rates))

    def channels(self) -> List[int]:
        return [self.upsample_initial_channel >> i for i in range(len(self.upsample_rates) + 1)]

    @classmethod
    def from_json(cls, text_or_dict) -> "HifiGanConfig":
        d = json.loads(text_or_dict) if isinstance(text_or_dict, str) else dict(text_or_dict)
        return cls(**{k: d[k] for k in cls.__dataclass_fields__ if k in d})


def state_dict_spec(cfg: HifiGanConfig) -> Dict[str, tuple]:
    """Generator.state_dict() names/shapes after remove_weight_norm (models.py:116-143)."""
    ch = cfg.channels()
    s = {"conv_pre.weight": (ch[0], cfg.num_mels, 7), "conv_pre.bias": (ch[0],)}
    nk = len(cfg.resblock_kernel_sizes)
    for i, k in enumerate(cfg.upsample_kernel_sizes):
        s[f"ups.{i}.weight"] = (ch[i], ch[i + 1], k)  # ConvTranspose1d: (in, out, k)
        s[f"ups.{i}.bias"] = (ch[i + 1],)
        for j, rk in enumerate(cfg.resblock_kernel_sizes):
            for grp in ("convs1", "convs2"):
                for m in range(3):
                    s[f"resblocks.{i * nk + j}.{grp}.{m}.weight"] = (ch[i + 1], ch[i + 1], rk)
                    s[f"resblocks.{i * nk + j}.{grp}.{m}.bias"] = (ch[i + 1],)
    s["conv_post.weight"] = (1, ch[-1], 7)
    s["conv_post.bias"] = (1,)
    return s


def synth_state_dict(cfg: HifiGanConfig, seed: int = 0, gain: float = 1.0) -> Dict[str, np.ndarray]:
    """Random generator weights (there is no network for generator_universal.pth.tar): N(0, gain/fan_in)
    conv weights so that activations stay O(1) through the 4 x 3 x 6 conv stack, small biases.
    numpy RandomState -> identical on every host."""
    rs = np.random.RandomState(seed)
    sd = {}
    for name, shape in state_dict_spec(cfg).items():
        if name.endswith(".bias"):
            sd[name] = (0.05 * rs.standard_normal(shape)).astype(np.float32)
        elif name.startswith("ups."):
            cin, _, k = shape
            u = cfg.upsample_rates[int(name.split(".")[1])]
            sd[name] = (rs.standard_normal(shape) * gain * (u / (cin * k)) ** 0.5).astype(np.float32)
        else:
            _, cin, k = shape
            g = gain * (0.1 if name.startswith("conv_post") else 1.0)  # keep tanh out of saturation
            sd[name] = (rs.standard_normal(shape) * g * (1.0 / (cin * k)) ** 0.5).astype(np.float32)
    return sd


def fold_weight_norm(sd: Dict[str, "torch.Tensor | np.ndarray"]) -> Dict[str, np.ndarray]:
    """Checkpoint form -> plain weights: w = g * v / ||v|| with the norm over all dims but 0, what
    torch.nn.utils.remove_weight_norm leaves in ``.weight`` (Synthesiser.__init__, __init__.py:31-33;
    weight_norm's default dim=0 also for ConvTranspose1d)."""
    out = {}
    for k, t in sd.items():
        a = t.detach().cpu().float().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)
        if k.endswith(".weight_g"):
            v = sd[k[:-2] + "_v"]
            v = v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float32)
            norm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=tuple(range(1, v.ndim)), keepdims=True))
            out[k[:-9] + ".weight"] = (a.astype(np.float64) * v / norm).astype(np.float32)
        elif k.endswith(".weight_v"):
            continue
        else:
            out[k] = a
    return out


Fs2VocConfigC = _lib.Fs2VocConfigC


def _config_to_c(cfg: HifiGanConfig, dtype: int) -> Fs2VocConfigC:
    c = Fs2VocConfigC()
    c.abi_version, c.dtype, c.n_mels = _lib.FS2_ABI_VERSION, dtype, cfg.num_mels
    c.initial_channel, c.n_stages = cfg.upsample_initial_channel, len(cfg.upsample_rates)
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        c.up_rates[i], c.up_kernels[i] = u, k
    c.n_kernels = len(cfg.resblock_kernel_sizes)
    for j, (k, ds) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
        c.rb_kernels[j] = k
        if len(ds) != 3:
            raise ValueError("resblock '1' has three dilations per kernel size")
        for m, d in enumerate(ds):
            c.rb_dilations[j][m] = d
    return c


_PRECISIONS = {"bf16": _lib.FS2_BF16, "fp32": _lib.FS2_F32, "fp16": _lib.FS2_F16}
_WAV_KINDS = {"int16": (_lib.FS2_WAV_I16, torch.int16), "float32": (_lib.FS2_WAV_F32, torch.float32)}


_DTYPE_NAMES = {v: k for k, v in _PRECISIONS.items()}


def decode_launch(code: int) -> tuple:
    """One code of fs2_voc_last_launches (include/fs2.h) -> ("conv", precision, MI16, CP, in_fp32, post, shift) or
    ("resblock", precision, form, channels, npairs, out_act, x_act): the template arguments of the kernel that ran and the
    argument flags that select its paths; precision as HifiGan spells it, flags as bools."""
    dt = _DTYPE_NAMES[(code >> 1) & 7]
    if code & 1:
        return ("resblock", dt, (code >> 4) & 1023, (code >> 14) & 255, (code >> 22) & 3, bool(code >> 24 & 1), bool(code >> 25 & 1))
    return ("conv", dt, (code >> 4) & 15, (code >> 8) & 1023, bool(code >> 18 & 1), bool(code >> 19 & 1), bool(code >> 20 & 1))


def wav_pack(wav: torch.Tensor, lengths: Optional[torch.Tensor], hop: int, dtype: str = "float32",
             out: Optional[torch.Tensor] = None):
    """fs2_op_wav_pack (include/fs2.h) on the current stream: wav (B, T*hop) fp32 device, lengths (B,) int32 device frame counts or
    None -> ``(packed, offsets)`` as ``HifiGan.synthesize_packed`` documents them.  ``out``: a flat device buffer of ``dtype`` with
    at least ``B*T*hop`` elements (the total is known on the device only); a smaller one is an error."""
    if dtype not in _WAV_KINDS:
        raise ValueError(f"dtype must be one of {sorted(_WAV_KINDS)}, got {dtype!r}")
    kind, tdt = _WAV_KINDS[dtype]
    if not wav.is_cuda or wav.dtype != torch.float32 or wav.dim() != 2 or not wav.is_contiguous():
        raise ValueError("wav must be a contiguous (B, T*hop) float32 device tensor")
    B, S = wav.shape
    if hop <= 0 or S % hop:
        raise ValueError(f"wav rows of {S} samples are no multiple of hop={hop}")
    if lengths is not None and (not lengths.is_cuda or lengths.dtype != torch.int32 or lengths.numel() != B
                                or not lengths.is_contiguous()):
        raise ValueError("lengths must be a contiguous (B,) int32 device tensor")
    if out is None:
        out = torch.empty(B * S, dtype=tdt, device=wav.device)
    elif not out.is_cuda or out.dtype != tdt or not out.is_contiguous() or out.device != wav.device:
        raise ValueError(f"out must be a contiguous {dtype} tensor on {wav.device}")
    offsets = torch.empty(B + 1, dtype=torch.int64, device=wav.device)
    lib = _lib.load()
    with torch.cuda.device(wav.device):
        st = lib.fs2_op_wav_pack(wav, lengths, B, S // hop, hop, kind, out, out.numel(), offsets, torch.cuda.current_stream(wav.device))
    _lib.check(st, None, f"op_wav_pack (capacity {out.numel()} for {B} x {S} samples)")
    return out, offsets


class HifiGan(_lib.Handle):
    """Device-resident generator.  ``state_dict`` may be the checkpoint form (weight_g / weight_v) or
    plain weights; names are the reference generator's own.

    ``precision``: "fp32" (parity mode, fp32 MFMA), "bf16" (throughput mode, the default) or "fp16": bf16's kernels, tiles and
    byte counts with every stored tensor (weights, the mel slab, the streams between launches, the stage means) in IEEE binary16
    - three more mantissa bits; stores saturate at +-65504.  Accumulation, biases, tanh and the wav are fp32 in all three."""
    _prefix = "fs2_voc"
    _load_what = "load_weight {}"

    def __init__(self, cfg: HifiGanConfig, state_dict, precision: str = "bf16", device="cuda:0"):
        self.cfg, self.device = cfg, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the HiFi-GAN generator runs on an MI355X only (no CPU fallback)")
        _lib.Handle.__init__(self)
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
        self.precision = precision
        self.dtype = _PRECISIONS[precision]
        cc = _config_to_c(cfg, self.dtype)
        with torch.cuda.device(self.device):  # no global set_device: the reference Synthesiser has no such side effect
            try:
                self._init(cfg, cc, state_dict)
            except Exception:
                self.close()
                raise
        self._last = None

    def _init(self, cfg, cc, state_dict):
        st = self.lib.fs2_voc_create(C.byref(cc), C.byref(self.handle))
        _lib.check(st, None, "fs2_voc_create")
        sd = fold_weight_norm(state_dict)
        spec = state_dict_spec(cfg)
        missing = [k for k in spec if k not in sd]
        if missing:
            raise KeyError(f"generator weights missing: {missing[:4]}{'...' if len(missing) > 4 else ''}")
        self.load_weights(spec, sd)
        self.hop = int(self.lib.fs2_voc_hop(self.handle))

    def _generate(self, mel: torch.Tensor, lengths: Optional[torch.Tensor], zero_pads: bool):
        mel = mel.to(self.device, torch.float32).contiguous()
        B, T, M = mel.shape
        if M != self.cfg.num_mels:
            raise ValueError(f"mel has {M} bins, generator wants {self.cfg.num_mels}")
        wav = (torch.zeros if zero_pads else torch.empty)(B, T * self.hop, dtype=torch.float32, device=self.device)
        ld = None if lengths is None else lengths.to(self.device, torch.int32).contiguous()
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):  # arena hipMalloc + launches must hit the engine's device
            self._check(self.lib.fs2_voc_synthesize(self.handle, mel, ld, B, T, wav, stream), "synthesize")
        self._last = (B, T)
        return wav, ld

    def synthesize(self, mel: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mel (B, T, n_mels) fp32 -> wav (B, T*hop) fp32 in [-1, 1]; with ``lengths`` (B,) every
        utterance is synthesised from its first lengths[b] frames only (samples past it are 0)."""
        return self._generate(mel, lengths, True)[0]

    def synthesize_packed(self, mel: torch.Tensor, lengths: Optional[torch.Tensor] = None, dtype: str = "float32",
                          out: Optional[torch.Tensor] = None):
        """``synthesize`` finished on the device (fs2_op_wav_pack right behind the generator, same stream): returns
        ``(packed, offsets)``, device tensors.  ``packed`` is flat, ``B*T*hop`` elements of capacity (or the caller's ``out``);
        utterance b's ``lengths[b]*hop`` samples are ``packed[offsets[b]:offsets[b+1]]``, ``offsets`` (B+1,) int64 and
        ``offsets[B]`` the total - what lies beyond it is not written.  dtype "int16": the samples ``Synthesiser.__call__`` returns,
        ``(wav * 32768.0).astype("int16")`` bit for bit; "float32": those divided by 32767 as ``int16_samples_to_float32`` does.
        The frame counts are never read by the host."""
        wav, ld = self._generate(mel, lengths, False)  # the pads are neither read nor written behind it: no memset
        return wav_pack(wav, ld, self.hop, dtype, out)

    def last_launches(self) -> list:
        """The kernel instantiation of every launch of the last ``synthesize``, in launch order (fs2_voc_last_launches), each as
        ``decode_launch`` spells it."""
        n = int(self.lib.fs2_voc_last_launches(self.handle, None, 0))
        if n < 0:
            raise RuntimeError("fs2_voc_last_launches failed")
        codes = (C.c_int32 * max(n, 1))()
        self.lib.fs2_voc_last_launches(self.handle, codes, n)
        return [decode_launch(codes[i]) for i in range(n)]

    def debug_stage(self, stage: int) -> torch.Tensor:
        B, T = self._last
        up = int(np.prod(self.cfg.upsample_rates[:stage])) if stage else 1
        t = torch.empty(B, T * up, self.cfg.channels()[stage], dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.fs2_voc_debug_copy(self.handle, stage, t, stream), "debug_copy")
        return t


class Synthesiser:
    """Drop-in for ``litfass.third_party.hifigan.Synthesiser`` (__init__.py:19-43): ``synth(mel)`` with
    mel ``(T, num_mels)`` returns int16 numpy ``(1, T*hop)``.  ``checkpoint`` is the path of a
    ``generator_*.pth.tar`` (``{"generator": state_dict}``) or a state_dict.  ``precision`` is HifiGan's ("bf16", "fp16", "fp32")."""

    def __init__(self, device="cuda:0", model="universal", checkpoint=None, config: Optional[HifiGanConfig] = None,
                 precision: str = "bf16"):
        self.device = device
        cfg = config or HifiGanConfig()
        if checkpoint is None:
            raise FileNotFoundError(f"generator_{model}.pth.tar is not shipped with the reference repository "
                                    "(a Git-LFS blob); pass checkpoint=<path or state_dict>")
        if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, "__fspath__"):
            checkpoint = torch.load(checkpoint, map_location="cpu")
        sd = checkpoint.get("generator", checkpoint)
        self.vocoder = HifiGan(cfg, sd, precision=precision, device=device)

    def __call__(self, mel):
        mel = torch.as_tensor(mel, dtype=torch.float32)
        # the cast runs on the device (fs2_op_wav_pack: numpy's own truncation and wrap, +1.0 -> -32768): 2 bytes per sample cross PCIe
        packed, _ = self.vocoder.synthesize_packed(mel.unsqueeze(0), None, "int16")
        return packed.cpu().numpy().reshape(1, -1)  # (1, T*hop)
