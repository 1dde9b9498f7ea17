"""Analysis front end: waveform -> log-mel spectrogram and frame energy on the device (the way back from audio).

``MelAnalyzer`` computes what the reference's ``TTSDataset.__getitem__`` / ``_create_variances`` compute per item on the CPU
with torchaudio and librosa (litfass/dataset/datasets.py:183-199, 369-380, 600-618, 630-648) - a centred Hann STFT magnitude
times a Slaney mel basis, ``log10(clamp(., 1e-6))``; the RMS of un-centred windows; the phone-level mean of a frame-level
variance - for a padded batch, in ``libfs2_hip.so`` through the ``fs2_mel_*`` C ABI (csrc/analysis.hip).  The semantics are
stated in include/fs2.h and DESIGN.md; there is no CPU fallback.

One deliberate difference: the reference divides by the peak unconditionally and gives NaN on an all-zero utterance; here such
an utterance keeps scale 1 (its mel is ``log(clip)``, its energy 0).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib


def _hz_to_mel(f):
    """The Slaney (Auditory Toolbox) mel scale: linear at 200/3 Hz per mel below 1 kHz, logarithmic above with 27 steps per
    factor 6.4."""
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), lin)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3.0))


def slaney_mel_edges(n_mels: int, fmin: float, fmax: float) -> np.ndarray:
    """The n_mels + 2 band edges in Hz: equally spaced on the Slaney mel scale from fmin to fmax."""
    return _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))


def slaney_mel_basis(sr: int = 22050, n_fft: int = 1024, n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = 8000.0) -> np.ndarray:
    """(n_mels, n_fft // 2 + 1) float32 triangular filters on the Slaney mel scale, each normalised by 2 / (f[m+2] - f[m])
    (unit area in Hz) - written from the published definition (Slaney's Auditory Toolbox; the scale is linear at 200/3 Hz per mel
    below 1 kHz and logarithmic above with step ln(6.4) / 27).

    NOT pinned against librosa's output: librosa is not a dependency of this project and was not available to compare with.
    It follows the same published definition (what ``librosa.filters.mel(htk=False, norm="slaney")`` documents), evaluated in
    float64 and rounded once; a user who needs a bit-for-bit librosa basis passes it to ``MelAnalyzer(mel_basis=...)``."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    if not (0 <= fmin < fmax <= sr / 2.0 + 1e-9):
        raise ValueError(f"need 0 <= fmin < fmax <= sr / 2, got fmin = {fmin}, fmax = {fmax}, sr = {sr}")
    edges = slaney_mel_edges(n_mels, fmin, fmax)
    freqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    lower = (freqs[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    upper = (edges[2:, None] - freqs[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    tri = np.maximum(0.0, np.minimum(lower, upper))
    return (tri * (2.0 / (edges[2:] - edges[:-2]))[:, None]).astype(np.float32)


# log="none": the mel itself, unclamped (what an accuracy figure is taken on)
_LOG_KINDS = {"log10": _lib.FS2_MEL_LOG10, "ln": _lib.FS2_MEL_LN, "none": _lib.FS2_MEL_LINEAR}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def segment_mean(values: torch.Tensor, durations: torch.Tensor, frames: Optional[torch.Tensor] = None, mean: float = 0.0,
                 std: float = 1.0, empty_value: float = 1e-7) -> torch.Tensor:
    """Phone-level reduction (datasets.py:631-648) on the device: values (B, T) fp32, durations (B, L) int, frames (B) valid
    frames per row or None -> (B, L): (mean of each phone's frames - mean) / std, (empty_value - mean) / std for an empty one."""
    if values.device.type != "cuda":
        raise RuntimeError("segment_mean runs on an MI355X only (no CPU fallback)")
    values = values.to(torch.float32).contiguous()
    dur = durations.to(values.device, torch.int32).contiguous()
    fr = None if frames is None else frames.to(values.device, torch.int32).contiguous()
    (B, T), L = values.shape, dur.shape[1]
    if dur.shape[0] != B or (fr is not None and tuple(fr.shape) != (B,)):
        raise ValueError(f"durations must be ({B}, L) and frames ({B},)")
    out = torch.empty(B, L, dtype=torch.float32, device=values.device)
    with torch.cuda.device(values.device):
        st = _lib.load().fs2_op_segment_mean(_ptr(values), _ptr(fr), _ptr(dur), B, T, L, C.c_float(empty_value), C.c_float(mean),
                                             C.c_float(std), _ptr(out), C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream))
    _lib.check(st, None, "op_segment_mean")
    return out


class MelAnalyzer:
    """Waveforms -> {"mel", "mel_lengths", "energy", "energy_lengths"} on the device.  The defaults are ``TTSDataset``'s
    (datasets.py:183-199); ``log="ln", clip=1e-5`` is the HiFi-GAN convention, ``log="none"`` returns the mel itself, unclamped.  ``mel_basis`` (n_mels, n_fft // 2 + 1) replaces
    the built-in :func:`slaney_mel_basis` (which is not pinned against librosa's output, see there)."""

    def __init__(self, sampling_rate: int = 22050, n_fft: int = 1024, win_length: int = 1024, hop_length: int = 256, n_mels: int = 80,
                 fmin: float = 0.0, fmax: Optional[float] = 8000.0, log: str = "log10", clip: float = 1e-6, mel_basis=None,
                 device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the analysis front end runs on an MI355X only (no CPU fallback)")
        if log not in _LOG_KINDS:
            raise ValueError(f"log must be one of {sorted(_LOG_KINDS)}, got {log!r}")
        self.lib = _lib.load()
        self.sampling_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels = sampling_rate, n_fft, win_length, hop_length, n_mels
        self.log, self.clip = log, float(clip)
        if mel_basis is None:
            mel_basis = slaney_mel_basis(sampling_rate, n_fft, n_mels, fmin, fmax)
        basis = np.ascontiguousarray(mel_basis.detach().cpu().numpy() if isinstance(mel_basis, torch.Tensor) else mel_basis, np.float32)
        if basis.shape != (n_mels, n_fft // 2 + 1):
            raise ValueError(f"mel_basis must be {(n_mels, n_fft // 2 + 1)}, got {basis.shape}")
        self.mel_basis = basis
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            st = self.lib.fs2_mel_create(_lib.FS2_ABI_VERSION, n_fft, win_length, hop_length, n_mels, C.c_float(self.clip),
                                         _LOG_KINDS[log], basis.ctypes.data_as(C.c_void_p),
                                         C.byref(self.handle))
        if st != _lib.FS2_OK:
            msg = self.lib.fs2_mel_last_error(self.handle).decode() if self.handle else ""
            self.close()
            raise RuntimeError(f"fs2_mel_create failed ({st}): {self.lib.fs2_status_string(st).decode()}: {msg}")
        self.tile_frames = int(self.lib.fs2_mel_tile_frames(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.fs2_mel_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _batch(self, wav, lengths):
        if isinstance(wav, (list, tuple)):
            arrs = [np.asarray(w.detach().cpu() if isinstance(w, torch.Tensor) else w, np.float32).reshape(-1) for w in wav]
            if not arrs or min(len(a) for a in arrs) < 1:
                raise ValueError("every utterance needs at least one sample")
            host = np.zeros((len(arrs), max(len(a) for a in arrs)), np.float32)
            for i, a in enumerate(arrs):
                host[i, :len(a)] = a
            if lengths is None:
                lengths = [len(a) for a in arrs]
            wav = torch.from_numpy(host)
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
            raise ValueError("wav must be a (B, S) tensor or a list of 1-D arrays")
        wav = wav.to(self.device, torch.float32).contiguous()
        if lengths is None:
            lengths = torch.full((wav.shape[0],), wav.shape[1], dtype=torch.int32)
        lengths = torch.as_tensor(lengths).to(self.device, torch.int32).contiguous()
        if tuple(lengths.shape) != (wav.shape[0],):
            raise ValueError(f"lengths must be ({wav.shape[0]},), got {tuple(lengths.shape)}")
        return wav, lengths

    def __call__(self, wav, lengths=None, peak_normalize: bool = True) -> Dict[str, torch.Tensor]:
        """wav: (B, S) device or host tensor, or a list of 1-D arrays (padded and uploaded); lengths (B) samples per row or None.
        Returns device tensors: mel (B, 1 + S // hop, n_mels) fp32 and energy (B, ceil(S / hop)) fp32, rows past an utterance's own
        count zero, with the counts as int32 (B,) mel_lengths / energy_lengths.  Samples at or past lengths[b] are never read."""
        wav, lengths = self._batch(wav, lengths)
        B, S = wav.shape
        hop = self.hop_length
        T_max, Te_max = 1 + S // hop, -(-S // hop)
        dev = self.device
        mel = torch.empty(B, T_max, self.n_mels, dtype=torch.float32, device=dev)
        en = torch.empty(B, Te_max, dtype=torch.float32, device=dev)
        mel_len = torch.empty(B, dtype=torch.int32, device=dev)
        en_len = torch.empty(B, dtype=torch.int32, device=dev)
        ws_bytes = int(self.lib.fs2_mel_ws_bytes(self.handle, B, S))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = self.lib.fs2_mel_run(self.handle, _ptr(wav), _ptr(lengths), B, S, int(bool(peak_normalize)), _ptr(mel), T_max, _ptr(en),
                                      Te_max, _ptr(mel_len), _ptr(en_len), _ptr(ws), ws_bytes,
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if st != _lib.FS2_OK:
            raise RuntimeError(f"fs2_mel_run failed ({st}): {self.lib.fs2_status_string(st).decode()}: "
                               f"{self.lib.fs2_mel_last_error(self.handle).decode()}")
        return {"mel": mel, "mel_lengths": mel_len, "energy": en, "energy_lengths": en_len}

    def targets(self, wavs: Sequence, durations: Sequence, stats: Optional[dict] = None, energy_level: str = "frame",
                peak_normalize: bool = True) -> List[dict]:
        """Per-utterance HOST items in the shape ``TTSDataset.__getitem__`` gives them (datasets.py:439-461): ``mel`` =
        mel[:sum(d)], ``duration`` = d (int64), ``variances["energy"]`` = the frame energy[:sum(d)] (energy_level "frame") or its
        phone-level mean (L,) (energy_level "phone"), normalised with stats["energy"]["mean" / "std"] when stats is given.  A
        caller adds "phones" and "speaker" to each item; ``frontend.collate`` then yields the batch keys
        ``Trainer.training_step`` reads (mel, duration, variances_energy)."""
        if energy_level not in ("frame", "phone"):
            raise ValueError(f"energy_level must be 'frame' or 'phone', got {energy_level!r}")
        if len(wavs) != len(durations):
            raise ValueError("one duration array per waveform")
        durs = [np.asarray(d.cpu() if isinstance(d, torch.Tensor) else d, np.int64).reshape(-1) for d in durations]
        mean, std = (float(stats["energy"]["mean"]), float(stats["energy"]["std"])) if stats is not None else (0.0, 1.0)
        out = self(list(wavs), peak_normalize=peak_normalize)
        mel_len, en_len = out["mel_lengths"].cpu().numpy(), out["energy_lengths"].cpu().numpy()
        if energy_level == "phone":
            L = max(len(d) for d in durs)
            dpad = np.zeros((len(durs), L), np.int32)
            for i, d in enumerate(durs):
                dpad[i, :len(d)] = d
            phone = segment_mean(out["energy"], torch.from_numpy(dpad), out["energy_lengths"], mean, std).cpu().numpy()
        mel, energy = out["mel"].cpu().numpy(), out["energy"].cpu().numpy()
        items = []
        for i, d in enumerate(durs):
            total = int(d.sum())
            if total > mel_len[i] or (energy_level == "frame" and total > en_len[i]):
                raise ValueError(f"utterance {i}: durations sum to {total} frames, the audio has {mel_len[i]} mel / {en_len[i]} energy frames")
            e = phone[i, :len(d)] if energy_level == "phone" else ((energy[i, :total] - np.float32(mean)) / np.float32(std)).astype(np.float32)
            items.append({"mel": mel[i, :total].copy(), "duration": d, "variances": {"energy": np.ascontiguousarray(e, np.float32)}})
        return items
