"""Augmentation of generated audio on the device: rational resampling, convolution with a caller-supplied impulse response and
Gaussian noise at a target SNR, applied to the packed waveform (``HifiGan.synthesize_packed``'s layout) before it crosses PCIe.

What the reference's ``SpeechGenerator`` does on the host, one utterance at a time, behind the vocoder: ``self.augmentations(audio,
sample_rate=...)`` = ``RoomSimulator`` + ``AddGaussianSNR`` (+ ``PitchShift``; generate.py:82-104, generator.py:197-201) and a resample
(generator.py:181).  The kernels (csrc/augment.hip) are written against the definitions in include/fs2.h, not against a library:

- the resampler follows torchaudio's published ``sinc_interp_hann`` definition (lowpass_filter_width 6, rolloff 0.99) and is NOT
  pinned against torchaudio's output;
- room *simulation* (geometry -> impulse response) is out of scope: impulse responses are an argument and none is shipped
  (``synthetic_rir`` is a test signal, not a room model);
- the noise follows ``AddGaussianSNR``'s rule ``noise_rms = signal_rms / 10^(snr / 20)``; ``PitchShift`` and VoiceFixer stay out.

Random decisions are made on the host from ONE ``numpy.random.Generator(seed)``: per call, for every stage that has decisions
(``RoomImpulse``, ``GaussianSNR``) in list order, for every utterance in order, three draws in this fixed order -
``random()`` (the stage applies iff it is < p), ``integers(n_rir)`` (which response; drawn and ignored by a noise stage) and
``uniform(min_snr_db, max_snr_db)`` (the SNR in dB; a response stage draws ``uniform(0, 1)`` and ignores it).  ``plan(B)`` makes
exactly these draws and needs no GPU.  The noise samples come from a seeded device ``torch.Generator`` (drawn at capacity size, so
the stream of numbers does not depend on the lengths), or are handed in as ``noise=``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
MAX_NEW, MAX_K, MAX_RIR = 640, 1024, 16384  # what fs2_op_wav_resample / fs2_op_wav_convolve support


def resample_params(orig_freq: int, new_freq: int) -> Tuple[int, int, int, int]:
    """``(orig, new, width, K)`` of include/fs2.h's definition: the rates over their gcd, the filter's half width in input samples
    and the taps per output phase."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("sample rates must be positive")
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * ROLLOFF
    width = int(math.ceil(LOWPASS_FILTER_WIDTH * orig / base))
    return orig, new, width, 2 * width + orig


def resample_table(orig_freq: int, new_freq: int) -> np.ndarray:
    """The (new, K) float64 table ``tab[p][q] = sinc(pi t) cos^2(pi t / (2 lpw)) base / orig`` with
    ``t = clip((-p / new + (q - width) / orig) * base, -lpw, lpw)`` (CPU only; the device takes it rounded once to float32)."""
    orig, new, width, K = resample_params(orig_freq, new_freq)
    base = min(orig, new) * ROLLOFF
    p = np.arange(new, dtype=np.float64)[:, None]
    q = np.arange(K, dtype=np.float64)[None, :]
    t = np.clip((-p / new + (q - width) / orig) * base, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = np.cos(np.pi * t / (2 * LOWPASS_FILTER_WIDTH)) ** 2
    return np.sinc(t) * window * (base / orig)  # np.sinc(t) = sin(pi t) / (pi t), 1 at 0


def resampled_length(n: int, orig: int, new: int) -> int:
    """ceil(new * n / orig) in integer arithmetic"""
    return -((-new * int(n)) // orig)


def synthetic_rir(n: int, decay: float, seed: int) -> np.ndarray:
    """A TEST SIGNAL, not a room model: ``n`` taps of Gaussian noise under ``exp(-decay * k)``, first tap 1, float32."""
    k = np.arange(n, dtype=np.float64)
    h = np.random.default_rng(seed).standard_normal(n) * np.exp(-decay * k)
    h[0] = 1.0
    return h.astype(np.float32)


# ---- the three operations on the current stream (thin wrappers of the C entry points; tensors on the device)
def _check_packed(packed, offsets):
    if not packed.is_cuda or packed.dtype != torch.float32 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("packed must be a flat contiguous float32 device tensor")
    if not offsets.is_cuda or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
        raise ValueError("offsets must be a contiguous (B + 1,) int64 device tensor")
    return offsets.numel() - 1


def _lib():
    from . import _lib as L
    return L


def wav_resample(packed: torch.Tensor, offsets: torch.Tensor, max_len: int, tab: torch.Tensor, orig: int, new: int, width: int,
                 out: Optional[torch.Tensor] = None):
    """fs2_op_wav_resample -> ``(packed, offsets, max_len)`` of the result; ``tab`` = ``resample_table`` as float32 on the device."""
    B = _check_packed(packed, offsets)
    m_max = resampled_length(max_len, orig, new)
    if out is None:
        out = torch.empty(max(B * m_max, 1), dtype=torch.float32, device=packed.device)
    out_off = torch.empty(B + 1, dtype=torch.int64, device=packed.device)
    L = _lib()
    with torch.cuda.device(packed.device):
        st = L.load().fs2_op_wav_resample(packed, offsets, B, max_len, tab, orig, new, width, out, out.numel(), out_off,
                                          torch.cuda.current_stream(packed.device))
    L.check(st, None, f"op_wav_resample ({orig} -> {new}, capacity {out.numel()} for {B} x {m_max})")
    return out, out_off, m_max


def wav_convolve(packed: torch.Tensor, offsets: torch.Tensor, max_len: int, rir: torch.Tensor, rir_len: torch.Tensor,
                 rir_index: torch.Tensor, mode: str = "same", out: Optional[torch.Tensor] = None):
    """fs2_op_wav_convolve -> ``(packed, offsets, max_len)``; ``rir`` (n_rir, R_max) float32, ``rir_len`` (n_rir,) int32,
    ``rir_index`` (B,) int32 (-1: copy), all on the device."""
    B = _check_packed(packed, offsets)
    if mode not in ("same", "full"):
        raise ValueError(f"mode must be 'same' or 'full', got {mode!r}")
    L = _lib()
    n_rir, R_max = rir.shape
    m_max = max_len if mode == "same" or max_len == 0 else max_len + R_max - 1
    if out is None:
        out = torch.empty(max(B * m_max, 1), dtype=torch.float32, device=packed.device)
    out_off = torch.empty(B + 1, dtype=torch.int64, device=packed.device)
    with torch.cuda.device(packed.device):
        st = L.load().fs2_op_wav_convolve(packed, offsets, B, max_len, rir, rir_len, rir_index, n_rir, R_max,
                                          L.FS2_CONV_SAME if mode == "same" else L.FS2_CONV_FULL, out, out.numel(), out_off,
                                          torch.cuda.current_stream(packed.device))
    L.check(st, None, f"op_wav_convolve (R_max {R_max}, {mode}, capacity {out.numel()} for {B} x {m_max})")
    return out, out_off, m_max


def wav_add_noise(packed: torch.Tensor, offsets: torch.Tensor, max_len: int, z: torch.Tensor, snr: torch.Tensor,
                  out: Optional[torch.Tensor] = None):
    """fs2_op_wav_add_noise -> ``(packed, scales)``; ``z`` packed float32 noise under the same offsets, ``snr`` (B,) float32 in dB
    (+inf: leave alone), ``out`` may be ``packed`` itself."""
    B = _check_packed(packed, offsets)
    L = _lib()
    lib = L.load()
    if out is None:
        out = torch.empty_like(packed)
    scales = torch.empty(B, dtype=torch.float32, device=packed.device)
    nbytes = int(lib.fs2_op_wav_add_noise_ws_bytes(B, max_len))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=packed.device)
    with torch.cuda.device(packed.device):
        st = lib.fs2_op_wav_add_noise(packed, offsets, B, max_len, z, snr, ws, ws.numel(), out, scales,
                                      torch.cuda.current_stream(packed.device))
    L.check(st, None, f"op_wav_add_noise ({B} x {max_len})")
    return out, scales


# ---- stages
class Resample:
    """``orig_freq -> new_freq``.  Equal rates drop the stage (``DeviceAugment`` leaves it out)."""
    random = False

    def __init__(self, orig_freq: int, new_freq: int):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.orig, self.new, self.width, self.K = resample_params(orig_freq, new_freq)
        if self.orig != self.new and (self.new > MAX_NEW or self.K > MAX_K):
            raise ValueError(f"resampling {orig_freq} -> {new_freq} (new = {self.new}, K = {self.K}) is outside new <= {MAX_NEW}, K <= {MAX_K}")

    def out_len(self, max_len: int) -> int:
        return resampled_length(max_len, self.orig, self.new)


class RoomImpulse:
    """Convolution with one of ``rirs`` (a list of 1-D arrays, applied as given: no rescaling), chosen per utterance, with probability
    ``p``.  ``mode="same"`` keeps the length (audiomentations' ``leave_length_unchanged``), ``"full"`` the whole tail."""
    random = True

    def __init__(self, rirs: Sequence[np.ndarray], p: float = 0.5, mode: str = "same"):
        rirs = [np.ascontiguousarray(r, dtype=np.float32) for r in rirs]
        if not rirs or any(r.ndim != 1 or not 1 <= r.shape[0] <= MAX_RIR for r in rirs):
            raise ValueError(f"rirs must be a non-empty list of 1-D arrays of 1..{MAX_RIR} taps")
        if mode not in ("same", "full"):
            raise ValueError(f"mode must be 'same' or 'full', got {mode!r}")
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must lie in [0, 1]")
        self.p, self.mode = float(p), mode
        self.R_max = max(r.shape[0] for r in rirs)
        self.bank = np.zeros((len(rirs), self.R_max), dtype=np.float32)
        for i, r in enumerate(rirs):
            self.bank[i, :r.shape[0]] = r
        self.lens = np.array([r.shape[0] for r in rirs], dtype=np.int32)

    def out_len(self, max_len: int) -> int:
        return max_len if self.mode == "same" or max_len == 0 else max_len + self.R_max - 1


class GaussianSNR:
    """``AddGaussianSNR``: white Gaussian noise at an SNR drawn uniformly in dB from [min_snr_db, max_snr_db], with probability ``p``."""
    random = True

    def __init__(self, min_snr_db: float, max_snr_db: float, p: float = 0.5):
        if not (math.isfinite(min_snr_db) and math.isfinite(max_snr_db) and min_snr_db <= max_snr_db):
            raise ValueError("need finite min_snr_db <= max_snr_db")
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must lie in [0, 1]")
        self.min_snr_db, self.max_snr_db, self.p = float(min_snr_db), float(max_snr_db), float(p)

    def out_len(self, max_len: int) -> int:
        return max_len


class DeviceAugment:
    """``aug(packed, offsets, fs, max_len) -> (packed, offsets, fs)``: the stages in list order on the current stream, without
    synchronising.  ``packed`` / ``offsets`` as ``HifiGan.synthesize_packed`` returns them (float32), ``max_len`` a host upper bound
    on any utterance's samples.  The result's ``packed`` has the stage chain's worst-case capacity; ``offsets[B]`` is the total."""

    def __init__(self, stages, seed: int = 0, device="cuda:0"):
        self.stages = [s for s in stages if not (isinstance(s, Resample) and s.orig == s.new)]
        for s in self.stages:
            if not isinstance(s, (Resample, RoomImpulse, GaussianSNR)):
                raise TypeError(f"not an augmentation stage: {s!r}")
        self.seed, self.device = int(seed), torch.device(device)
        self.rng = np.random.default_rng(self.seed)
        self._dev = None   # per-stage device constants, uploaded at the first call
        self._gen = None   # the device generator of the noise

    # -- host side (no GPU)
    def plan(self, B: int) -> List[Optional[dict]]:
        """The next call's decisions, one entry per stage (None for a stage without any): ``{"apply": bool (B,), "rir": int32 (B,)
        (-1 where the stage does not apply), "snr": float32 (B,) (+inf where it does not apply)}``.  Advances the generator."""
        plans = []
        for s in self.stages:
            if not s.random:
                plans.append(None)
                continue
            apply, rir, snr = np.zeros(B, bool), np.full(B, -1, np.int32), np.full(B, np.inf, np.float32)
            is_rir = isinstance(s, RoomImpulse)
            for b in range(B):
                u = self.rng.random()
                r = int(self.rng.integers(s.bank.shape[0] if is_rir else 1))
                v = self.rng.uniform(s.min_snr_db, s.max_snr_db) if not is_rir else self.rng.uniform(0.0, 1.0)
                apply[b] = u < s.p
                if apply[b] and is_rir:
                    rir[b] = r
                if apply[b] and not is_rir:
                    snr[b] = np.float32(v)
            plans.append({"apply": apply, "rir": rir, "snr": snr})
        return plans

    def out_fs(self, fs: int) -> int:
        for s in self.stages:
            if isinstance(s, Resample):
                if fs != s.orig_freq:
                    raise ValueError(f"Resample({s.orig_freq}, {s.new_freq}) got audio at {fs} Hz")
                fs = s.new_freq
        return fs

    def out_len(self, max_len: int) -> int:
        """the worst-case samples per utterance behind the whole chain"""
        for s in self.stages:
            max_len = s.out_len(max_len)
        return max_len

    # -- device side
    def _constants(self):
        if self._dev is None:
            dev = []
            for s in self.stages:
                if isinstance(s, Resample):
                    dev.append(torch.from_numpy(resample_table(s.orig_freq, s.new_freq).astype(np.float32)).to(self.device))
                elif isinstance(s, RoomImpulse):
                    dev.append((torch.from_numpy(s.bank).to(self.device), torch.from_numpy(s.lens).to(self.device)))
                else:
                    dev.append(None)
            self._dev = dev
        return self._dev

    def _noise(self, numel: int) -> torch.Tensor:
        if self._gen is None:
            self._gen = torch.Generator(device=self.device)
            self._gen.manual_seed(self.seed)
        return torch.randn(numel, generator=self._gen, dtype=torch.float32, device=self.device)

    def __call__(self, packed: torch.Tensor, offsets: torch.Tensor, fs: int, max_len: int, noise: Optional[torch.Tensor] = None,
                 plan: Optional[list] = None):
        B = _check_packed(packed, offsets)
        if packed.device != self.device:
            raise ValueError(f"packed is on {packed.device}, the augmentation on {self.device}")
        fs_out = self.out_fs(fs)
        plan = self.plan(B) if plan is None else plan
        max_len = int(max_len)
        own = False  # whether `packed` is a buffer of this call (the caller's is never written)
        for s, c, pl in zip(self.stages, self._constants(), plan):
            if isinstance(s, Resample):
                packed, offsets, max_len = wav_resample(packed, offsets, max_len, c, s.orig, s.new, s.width)
            elif isinstance(s, RoomImpulse):
                idx = torch.from_numpy(pl["rir"]).to(self.device, non_blocking=True)
                packed, offsets, max_len = wav_convolve(packed, offsets, max_len, c[0], c[1], idx, s.mode)
            else:
                snr = torch.from_numpy(pl["snr"]).to(self.device, non_blocking=True)
                z = noise if noise is not None else self._noise(max(B * max_len, 1))
                if z.numel() < packed.numel() and z.numel() < B * max_len:
                    raise ValueError(f"noise has {z.numel()} samples, the packed buffer may hold {B * max_len}")
                packed, self.last_scales = wav_add_noise(packed, offsets, max_len, z, snr, out=packed if own else None)
            own = True
        return packed, offsets, fs_out
