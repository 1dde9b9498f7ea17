"""Analysis front end: waveform -> log-mel spectrogram and frame energy on the device (the way back from audio).

``MelAnalyzer`` computes what the reference's ``TTSDataset.__getitem__`` / ``_create_variances`` compute per item on the CPU
with torchaudio and librosa (litfass/dataset/datasets.py:183-199, 369-380, 600-618, 630-648) - a centred Hann STFT magnitude
times a Slaney mel basis, ``log10(clamp(., 1e-6))``; the RMS of un-centred windows; the phone-level mean of a frame-level
variance - for a padded batch, in ``libfs2_hip.so`` through the ``fs2_mel_*`` C ABI (csrc/analysis.hip).  The semantics are
stated in include/fs2.h and DESIGN.md; there is no CPU fallback.

One deliberate difference: the reference divides by the peak unconditionally and gives NaN on an all-zero utterance; here such
an utterance keeps scale 1 (its mel is ``log(clip)``, its energy 0).

Training targets (include/fs2.h "Training targets from audio"): ``MelAnalyzer.snr`` is the reference's windowed WADA estimate
(``SNR.windowed_wada``, litfass/dataset/snr.py), :func:`finish_contour` what ``_create_variances`` does to the SNR and pitch
contours (silent phones and unvoiced frames become missing, gaps are filled by ``np.interp``, datasets.py:576-598), and
``MelAnalyzer.items`` the items of ``TTSDataset.__getitem__`` with their priors (:412-435).  Three things to know:

* the WADA table is an argument - the project ships none.  It is Kim & Stern's table for gamma shape 0.4; a litfass installation has
  it as ``litfass/data/wada_values.npy``: ``MelAnalyzer(wada_table=np.load(...))``.
* the raw F0 contour is the caller's or the project's own: ``items(pitch=...)`` takes it per utterance, one value per frame, 0
  where unvoiced, as pyworld's dio + stonemask return it (what the reference uses), or tracks it on the device with
  ``pitch="track"`` (``MelAnalyzer.pitch``: YIN, written from the published definition and NOT pinned against pyworld's output -
  its contours differ from DIO + StoneMask's, so ``stats`` must come from the tracker that made the contours they normalise).
* two deliberate differences: the reference's closing energy split ``10 log10(dSigEng / dNoiseEng)`` (the estimate again, to
  float64 rounding) is not reproduced, and phone-level means average the original frames (the reference writes them in place
  while reading, which differs only after leading zero-duration phones).

Variance transforms (include/fs2.h "CWT and log variance targets"): :func:`cwt_decompose` is the reference's ``CWT.decompose``
(litfass/dataset/cwt.py) and ``items(transforms=...)`` its transform step (datasets.py:641-648), so the class-default
configuration - phone-level variances, the pitch as a CWT item - comes from audio, durations and silence flags too.  The transform is
written from the definition of ``scipy.signal.cwt`` / ``ricker`` as SciPy 1.14 published them and is NOT pinned against their output:
SciPy removed both in 1.15.
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
        st = _lib.load().fs2_op_segment_mean(values, fr, dur, B, T, L, empty_value, mean, std, out, torch.cuda.current_stream(values.device))
    _lib.check(st, None, "op_segment_mean")
    return out


def _int_mat(rows, B, width, what):
    """a list of per-utterance integer arrays, or a (B, width) array / tensor -> a padded (B, width) int32 host array"""
    if isinstance(rows, torch.Tensor):
        rows = rows.detach().cpu().numpy()
    if isinstance(rows, np.ndarray) and rows.ndim == 2:
        out = np.ascontiguousarray(rows, np.int32)
    else:
        rows = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r).astype(np.int32).reshape(-1) for r in rows]
        out = np.zeros((len(rows), max([width] + [len(r) for r in rows])), np.int32)
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
    if out.shape[0] != B or (width and out.shape[1] != width):
        raise ValueError(f"{what} must be ({B}, {width or 'L'}), got {out.shape}")
    return out


def finish_contour(values: torch.Tensor, durations, silent=None, frames=None, zero_is_missing: bool = False,
                   all_missing_value: float = 0.0, mean: float = 0.0, std: float = 1.0) -> Dict[str, torch.Tensor]:
    """Contour finishing (datasets.py:576-598, ``_interpolate``) on the device: values (B, T) fp32 the raw frame contour, durations
    (B, L) int (or a list of arrays), silent (B, L) non-zero = silent phone or None, frames (B) valid frames per row or None ->
    {"values" (B, T): frames of silent phones, NaN and (zero_is_missing) zeros filled by np.interp from the present ones, or
    all_missing_value where nothing is present, then (. - mean) / std, zeros from frames[b] on; "frames" (B) int32 =
    min(sum of durations, frames); "prior" (B) the mean of the filled contour over the frames of non-silent phones, before
    normalisation}.  Pitch: zero_is_missing=True, all_missing_value=1e-7; SNR: the defaults.  T <= 4096, L <= 2048."""
    if values.device.type != "cuda":
        raise RuntimeError("finish_contour runs on an MI355X only (no CPU fallback)")
    values = values.to(torch.float32).contiguous()
    B, T = values.shape
    dur = torch.from_numpy(_int_mat(durations, B, 0, "durations")).to(values.device)
    L = dur.shape[1]
    sil = None if silent is None else torch.from_numpy(_int_mat(silent, B, L, "silent")).to(values.device)
    fr = None if frames is None else torch.as_tensor(frames).to(values.device, torch.int32).contiguous()
    if fr is not None and tuple(fr.shape) != (B,):
        raise ValueError(f"frames must be ({B},), got {tuple(fr.shape)}")
    out = torch.empty(B, T, dtype=torch.float32, device=values.device)
    fout = torch.empty(B, dtype=torch.int32, device=values.device)
    prior = torch.empty(B, dtype=torch.float32, device=values.device)
    with torch.cuda.device(values.device):
        st = _lib.load().fs2_op_contour_finish(values, fr, dur, sil, B, T, L, int(bool(zero_is_missing)), all_missing_value, mean, std, out,
                                               fout, prior, torch.cuda.current_stream(values.device))
    if st == _lib.FS2_ERR_SHAPE:
        raise ValueError(f"finish_contour holds one utterance in LDS: T = {T} <= 4096 frames and L = {L} <= 2048 phones")
    _lib.check(st, None, "op_contour_finish")
    return {"values": out, "frames": fout, "prior": prior}


def masked_row_mean(values: torch.Tensor, counts=None, skip=None) -> torch.Tensor:
    """values (B, N) fp32, counts (B) or None, skip (B, N) non-zero = leave out, or None -> (B,): the mean of each row's first
    counts[b] entries that are not skipped, NaN for none (the priors of datasets.py:412-435)."""
    if values.device.type != "cuda":
        raise RuntimeError("masked_row_mean runs on an MI355X only (no CPU fallback)")
    values = values.to(torch.float32).contiguous()
    B, N = values.shape
    cn = None if counts is None else torch.as_tensor(counts).to(values.device, torch.int32).contiguous()
    sk = None if skip is None else torch.as_tensor(skip).to(values.device, torch.int32).contiguous()
    if (cn is not None and tuple(cn.shape) != (B,)) or (sk is not None and tuple(sk.shape) != (B, N)):
        raise ValueError(f"counts must be ({B},) and skip ({B}, {N})")
    out = torch.empty(B, dtype=torch.float32, device=values.device)
    with torch.cuda.device(values.device):
        st = _lib.load().fs2_op_masked_row_mean(values, cn, sk, B, N, out, torch.cuda.current_stream(values.device))
    _lib.check(st, None, "op_masked_row_mean")
    return out


def cwt_decompose(values: torch.Tensor, counts=None, n_scales: int = 10, tau: float = 0.2833425) -> Dict[str, torch.Tensor]:
    """``CWT.decompose`` (litfass/dataset/cwt.py:30-46) on the device: values (B, S) fp32 a finished contour per row (frame level
    from :func:`finish_contour`, phone level from :func:`segment_mean`), counts (B) entries per row or None -> {"original_signal"
    (B, S): values with an exact 0 replaced by 1e-7; "signal" (B, S): its log; "spectrogram" (B, S, n_scales): the Ricker CWT of the
    normalised signal at the widths 2^(i + 1) tau, each scale times (i + 2.5)^(-5/2); "mean", "std" (B,): of the signal over the
    row's own entries}, zeros at and past a row's count.  S <= 4096.  The definition is stated in include/fs2.h.

    NOT pinned against ``scipy.signal.cwt``'s output: SciPy removed ``cwt`` and ``ricker`` in 1.15 and they were not available to
    compare with.  It follows their definition as SciPy 1.14 published it, in float64, rounded once."""
    if values.device.type != "cuda":
        raise RuntimeError("cwt_decompose runs on an MI355X only (no CPU fallback)")
    values = values.to(torch.float32).contiguous()
    if values.dim() != 2:
        raise ValueError(f"values must be (B, S), got {tuple(values.shape)}")
    B, S = values.shape
    cn = None if counts is None else torch.as_tensor(counts).to(values.device, torch.int32).contiguous()
    if cn is not None and tuple(cn.shape) != (B,):
        raise ValueError(f"counts must be ({B},), got {tuple(cn.shape)}")
    # zeros, not empty: a row whose count is 0 is not written
    orig, sig = torch.zeros(B, S, dtype=torch.float32, device=values.device), torch.zeros(B, S, dtype=torch.float32, device=values.device)
    spec = torch.zeros(B, S, max(0, int(n_scales)), dtype=torch.float32, device=values.device)
    ms = torch.empty(B, 2, dtype=torch.float32, device=values.device)
    with torch.cuda.device(values.device):
        st = _lib.load().fs2_op_cwt_decompose(values, cn, B, S, int(n_scales), float(tau), orig, sig, spec, ms,
                                              torch.cuda.current_stream(values.device))
    if st == _lib.FS2_ERR_SHAPE:
        raise ValueError(f"cwt_decompose holds one utterance in LDS: S = {S} <= 4096 entries (and B = {B} <= 65535 rows)")
    _lib.check(st, None, "op_cwt_decompose")
    return {"original_signal": orig, "signal": sig, "spectrogram": spec, "mean": ms[:, 0].contiguous(), "std": ms[:, 1].contiguous()}


_TRANSFORMS = ("none", "log", "cwt")


def _check_transforms(transforms, variances) -> List[str]:
    """items' ``transforms`` argument -> one of "none", "log", "cwt" per variance (None: "none" for each)"""
    transforms = ["none"] * len(variances) if transforms is None else list(transforms)
    if len(transforms) != len(variances) or any(t not in _TRANSFORMS for t in transforms):
        raise ValueError(f"transforms must name one of {_TRANSFORMS} for each of {list(variances)}, got {transforms}")
    return transforms


class MelAnalyzer(_lib.Handle):
    """Waveforms -> {"mel", "mel_lengths", "energy", "energy_lengths"} on the device.  The defaults are ``TTSDataset``'s
    (datasets.py:183-199); ``log="ln", clip=1e-5`` is the HiFi-GAN convention, ``log="none"`` returns the mel itself, unclamped.  ``mel_basis`` (n_mels, n_fft // 2 + 1) replaces
    the built-in :func:`slaney_mel_basis` (which is not pinned against librosa's output, see there)."""
    _prefix = "fs2_mel"

    def __init__(self, sampling_rate: int = 22050, n_fft: int = 1024, win_length: int = 1024, hop_length: int = 256, n_mels: int = 80,
                 fmin: float = 0.0, fmax: Optional[float] = 8000.0, log: str = "log10", clip: float = 1e-6, mel_basis=None,
                 device="cuda:0", wada_table=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the analysis front end runs on an MI355X only (no CPU fallback)")
        if log not in _LOG_KINDS:
            raise ValueError(f"log must be one of {sorted(_LOG_KINDS)}, got {log!r}")
        _lib.Handle.__init__(self)
        self.sampling_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels = sampling_rate, n_fft, win_length, hop_length, n_mels
        self.log, self.clip = log, float(clip)
        if mel_basis is None:
            mel_basis = slaney_mel_basis(sampling_rate, n_fft, n_mels, fmin, fmax)
        basis = np.ascontiguousarray(mel_basis.detach().cpu().numpy() if isinstance(mel_basis, torch.Tensor) else mel_basis, np.float32)
        if basis.shape != (n_mels, n_fft // 2 + 1):
            raise ValueError(f"mel_basis must be {(n_mels, n_fft // 2 + 1)}, got {basis.shape}")
        self.mel_basis = basis
        with torch.cuda.device(self.device):
            st = self.lib.fs2_mel_create(_lib.FS2_ABI_VERSION, n_fft, win_length, hop_length, n_mels, self.clip, _LOG_KINDS[log],
                                         basis.ctypes.data_as(C.c_void_p), C.byref(self.handle))
        if st != _lib.FS2_OK:  # the handle comes back on failure too, for its message
            try:
                self._check(st, "fs2_mel_create")
            finally:
                self.close()
        self.tile_frames = int(self.lib.fs2_mel_tile_frames(self.handle))
        self.wada_table = None
        if wada_table is not None:
            try:
                self.set_wada_table(wada_table)
            except Exception:
                self.close()
                raise

    def set_wada_table(self, table, db_lo: float = -20.0):
        """The WADA table ``snr`` looks its statistic up in: g[i] for db_lo + i dB, 2 to 512 finite values (the reference's:
        ``np.load("litfass/data/wada_values.npy")``, 121 values from -20 dB).  May be called again."""
        table = np.ascontiguousarray(table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table, np.float64).reshape(-1)
        with torch.cuda.device(self.device):
            st = self.lib.fs2_mel_set_snr_table(self.handle, table.ctypes.data_as(C.c_void_p), len(table), db_lo)
        self._check(st, "fs2_mel_set_snr_table")
        self.wada_table = table

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
            st = self.lib.fs2_mel_run(self.handle, wav, lengths, B, S, int(bool(peak_normalize)), mel, T_max, en, Te_max, mel_len, en_len,
                                      ws, ws_bytes, torch.cuda.current_stream(dev))
        self._check(st, "fs2_mel_run")
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

    def snr(self, wav, lengths=None, peak_normalize: bool = True) -> Dict[str, torch.Tensor]:
        """The windowed WADA estimate (``SNR.windowed_wada(window=win_length, stride=hop / win_length, use_samples=True)``): wav and
        lengths as in ``__call__`` -> device tensors snr (B, ceil(S / hop)) fp32 - the reference's ``snr + 20`` per hop over
        win_length-sample windows, NaN where it has NaN, rows past an utterance's own count zero - and snr_lengths (B) int32."""
        if self.wada_table is None:
            raise RuntimeError("MelAnalyzer.snr needs the WADA table, and the project ships none: pass wada_table= or call "
                               "set_wada_table(np.load('<litfass>/litfass/data/wada_values.npy')) - Kim & Stern's table for gamma shape 0.4")
        wav, lengths = self._batch(wav, lengths)
        B, S = wav.shape
        Te_max = -(-S // self.hop_length)
        dev = self.device
        out = torch.empty(B, Te_max, dtype=torch.float32, device=dev)
        out_len = torch.empty(B, dtype=torch.int32, device=dev)
        ws_bytes = int(self.lib.fs2_mel_ws_bytes(self.handle, B, S))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = self.lib.fs2_mel_snr(self.handle, wav, lengths, B, S, int(bool(peak_normalize)), out, Te_max, out_len, ws, ws_bytes,
                                      torch.cuda.current_stream(dev))
        self._check(st, "fs2_mel_snr")
        return {"snr": out, "snr_lengths": out_len}

    def pitch(self, wav, lengths=None, f0_floor: float = 71.0, f0_ceil: float = 800.0, threshold: float = 0.1,
              return_cmnd: bool = False) -> Dict[str, torch.Tensor]:
        """The raw F0 contour by YIN (de Cheveigne & Kawahara 2002; the definition is stated in include/fs2.h "F0 tracking"): wav
        and lengths as in ``__call__`` -> device tensors f0 (B, 1 + S // hop) fp32 in Hz - 0 where unvoiced, frame t centred on
        sample t * hop, rows past an utterance's own count zero: pyworld's contract, what ``finish_contour(zero_is_missing=True)``
        takes -, f0_lengths (B) int32, dmin (B, 1 + S // hop) the normalised difference at the picked lag (its minimum over the lag
        range on an unvoiced frame) and, with return_cmnd, cmnd (B, 1 + S // hop, tau_max + 2) the whole normalised difference
        function (diagnostic).  Lags run from max(2, floor(sr / f0_ceil)) to ceil(sr / f0_floor); the defaults are pyworld's range.

        NOT pinned against pyworld's output: pyworld is not a dependency of this project and was not available to compare with.
        The contours differ from DIO + StoneMask's; statistics (mean / std, bins) must come from the same tracker as the contours
        they normalise.  The definition is scale-invariant, so there is no peak normalisation."""
        wav, lengths = self._batch(wav, lengths)
        B, S = wav.shape
        dev = self.device
        tau_min, tau_max = C.c_int32(), C.c_int32()
        self._check(self.lib.fs2_mel_pitch_lags(self.handle, self.sampling_rate, f0_floor, f0_ceil, C.byref(tau_min), C.byref(tau_max)),
                    "fs2_mel_pitch_lags")
        Tf_max, n_lags = 1 + S // self.hop_length, tau_max.value + 2
        f0 = torch.empty(B, Tf_max, dtype=torch.float32, device=dev)
        dmin = torch.empty(B, Tf_max, dtype=torch.float32, device=dev)
        f0_len = torch.empty(B, dtype=torch.int32, device=dev)
        cmnd = torch.empty(B, Tf_max, n_lags, dtype=torch.float32, device=dev) if return_cmnd else None
        with torch.cuda.device(dev):
            st = self.lib.fs2_mel_pitch(self.handle, wav, lengths, B, S, self.sampling_rate, f0_floor, f0_ceil, threshold, f0, Tf_max, f0_len,
                                        dmin, cmnd, n_lags, torch.cuda.current_stream(dev))
        self._check(st, "fs2_mel_pitch")
        out = {"f0": f0, "f0_lengths": f0_len, "dmin": dmin}
        if return_cmnd:
            out["cmnd"] = cmnd
        return out

    def items(self, wavs: Sequence, durations: Sequence, silent: Optional[Sequence] = None, pitch=None,
              stats: Optional[dict] = None, variances: Sequence[str] = ("pitch", "energy", "snr"),
              levels: Sequence[str] = ("frame",) * 3, priors: Sequence[str] = (), peak_normalize: bool = True,
              pitch_options: Optional[dict] = None, transforms: Optional[Sequence[str]] = None) -> List[dict]:
        """Per-utterance HOST items in the shape ``TTSDataset.__getitem__`` gives them (datasets.py:398-463): ``mel``, ``duration``,
        ``variances`` {name: (sum(d),) at level "frame", (L,) at level "phone"}, ``priors`` {name: float}, ``silence_mask``
        (sum(d),) and ``unexpanded_silence_mask`` (L,) bool.  A caller adds "phones" and "speaker" and hands the list to
        ``frontend.collate``.  ``silent``: per utterance, True where a phone is silence (None: none is).  ``pitch``: per utterance
        the raw F0 contour, one value per frame and 0 where unvoiced (pyworld's output), or the string "track": the contours are
        then tracked on the device by ``self.pitch(wavs, **pitch_options)`` and go to the finishing without leaving it (see
        ``pitch`` on what that tracker is and is not; ``stats["pitch"]`` must belong to it) - one of the two is required when "pitch"
        is asked for.  "snr" needs the WADA table.  ``energy`` gets no silence handling, as in the reference.
        ``stats`` {name: {"mean", "std"}} normalises; priors are taken before normalisation (over non-silent frames, or phones at
        level "phone"; "duration": over non-silent phones).
        ``transforms``: per variance "none" (the default for each), "log" or "cwt" - the reference's ``variance_transforms``
        (datasets.py:641-648; its class default is ("cwt", "none", "none") at levels ("phone",) * 3).  A transformed variance is
        taken UNNORMALISED, ``stats`` are not applied to it (the reference's ``elif``), and priors are taken before any transform.
        "log": the natural log of the variance.  "cwt": ``variances[name]`` is the dict :func:`cwt_decompose` describes, per
        utterance - "signal", "original_signal" (n,), "spectrogram" (n, 10), "mean", "std" (np.float32) over the n = L phone means
        (1e-7 for an empty phone) at level "phone", the n = sum(d) frames otherwise - which ``frontend.collate`` flattens to the
        ``variances_<name>_signal`` / ``_spectrogram`` / ``_mean`` / ``_std`` that ``Trainer.training_step`` reads."""
        variances, levels, priors = list(variances), list(levels), list(priors)
        if len(levels) != len(variances) or any(lv not in ("frame", "phone") for lv in levels):
            raise ValueError(f"levels must name 'frame' or 'phone' for each of {variances}, got {levels}")
        transforms = _check_transforms(transforms, variances)
        for v in variances:
            if v not in ("pitch", "energy", "snr"):
                raise ValueError(f"variance {v!r} is none of 'pitch', 'energy', 'snr'")
        for p in priors:
            if p != "duration" and p not in variances:
                raise ValueError(f"prior {p!r} is neither 'duration' nor one of the variances {variances}")
        if "pitch" in variances and pitch is None:
            raise ValueError("variances includes 'pitch': pass pitch= (the raw F0 contour per utterance, 0 where unvoiced)")
        track = isinstance(pitch, str)
        if track and pitch != "track":
            raise ValueError(f"pitch must be the F0 contours or 'track', got {pitch!r}")
        if pitch_options is not None and not track:
            raise ValueError("pitch_options belongs to pitch='track'")
        if len(wavs) != len(durations) or (silent is not None and len(silent) != len(wavs)) or (pitch is not None and not track and len(pitch) != len(wavs)):
            raise ValueError("one duration array (and silent / pitch array) per waveform")
        B = len(wavs)
        durs = [np.asarray(d.cpu() if isinstance(d, torch.Tensor) else d, np.int64).reshape(-1) for d in durations]
        sils = [np.zeros(len(d), bool) if silent is None else np.asarray(silent[i]).reshape(-1) != 0 for i, d in enumerate(durs)]
        if any(len(s) != len(d) for s, d in zip(sils, durs)):
            raise ValueError("silent must have one flag per phone")
        totals = [int(np.maximum(d, 0).sum()) for d in durs]
        dev = self.device
        dpad = _int_mat(durs, B, 0, "durations")
        L = dpad.shape[1]
        spad = _int_mat(sils, B, L, "silent")
        dur_t = torch.from_numpy(dpad)
        n_phones = torch.tensor([len(d) for d in durs], dtype=torch.int32, device=dev)
        frame_sil = [np.repeat(s, np.maximum(d, 0)) for s, d in zip(sils, durs)]
        out = self(list(wavs), peak_normalize=peak_normalize)
        mel_len, en_len = out["mel_lengths"].cpu().numpy(), out["energy_lengths"].cpu().numpy()
        for i, total in enumerate(totals):
            if total > mel_len[i] or total > en_len[i]:
                raise ValueError(f"utterance {i}: durations sum to {total} frames, the audio has {mel_len[i]} mel / {en_len[i]} energy frames")
            if pitch is not None and not track and "pitch" in variances and len(pitch[i]) < total:
                raise ValueError(f"utterance {i}: durations sum to {total} frames, the F0 contour has {len(pitch[i])}")
        tot_dev = torch.tensor(totals, dtype=torch.int32, device=dev)
        fs_pad = np.zeros((B, max(1, out["energy"].shape[1])), np.int32)  # frame-level silence, for the energy prior
        for i, f in enumerate(frame_sil):
            fs_pad[i, :len(f)] = f
        var_host, prior_host = {}, {}
        for name, level, transform in zip(variances, levels, transforms):
            normalise = stats is not None and transform == "none"  # a transformed variance is taken unnormalised
            mean, std = (float(stats[name]["mean"]), float(stats[name]["std"])) if normalise else (0.0, 1.0)
            phone = level == "phone"
            if name == "energy":
                frame_vals, frames = out["energy"], tot_dev
                if phone:
                    vals = segment_mean(frame_vals, dur_t, frames, mean, std)
                else:
                    vals = (frame_vals - mean) / std
                fprior = None
            else:
                if name == "snr":
                    s = self.snr(list(wavs), peak_normalize=peak_normalize)
                    raw, raw_len, kw = s["snr"], s["snr_lengths"], dict(zero_is_missing=False, all_missing_value=0.0)
                elif track:  # (its frame count is the mel's, checked against the durations above)
                    p = self.pitch(list(wavs), **(pitch_options or {}))
                    raw, raw_len, kw = p["f0"], p["f0_lengths"], dict(zero_is_missing=True, all_missing_value=1e-7)
                else:
                    f0 = [np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p, np.float32).reshape(-1) for p in pitch]
                    host = np.zeros((B, max(1, max(len(p) for p in f0))), np.float32)
                    for i, p in enumerate(f0):
                        host[i, :len(p)] = p
                    raw, raw_len = torch.from_numpy(host).to(dev), torch.tensor([len(p) for p in f0], dtype=torch.int32, device=dev)
                    kw = dict(zero_is_missing=True, all_missing_value=1e-7)
                fin = finish_contour(raw, dpad, spad, raw_len, mean=0.0 if phone else mean, std=1.0 if phone else std, **kw)
                frame_vals, frames, fprior = fin["values"], fin["frames"], fin["prior"]
                vals = segment_mean(frame_vals, dur_t, frames, mean, std) if phone else frame_vals
            if name in priors:
                if phone:  # over the phone means of the non-silent phones, un-normalised
                    pm = segment_mean(out["energy"] if name == "energy" else frame_vals, dur_t, frames)
                    pr = masked_row_mean(pm, n_phones, torch.from_numpy(spad))
                elif fprior is None:
                    pr = masked_row_mean(frame_vals, tot_dev, torch.from_numpy(fs_pad[:, :frame_vals.shape[1]]))
                else:
                    pr = fprior
                prior_host[name] = pr.cpu().numpy()
            if transform == "cwt":
                dec = cwt_decompose(vals, n_phones if phone else frames)
                var_host[name] = {k: v.cpu().numpy() for k, v in dec.items()}
                continue
            if transform == "log":  # in fp64, rounded once: what "signal" is in a CWT item
                vals = torch.log(vals.to(torch.float64)).to(torch.float32)
            var_host[name] = vals.cpu().numpy()
        if "duration" in priors:
            prior_host["duration"] = masked_row_mean(torch.from_numpy(dpad).to(dev, torch.float32), n_phones, torch.from_numpy(spad)).cpu().numpy()
        mel = out["mel"].cpu().numpy()
        def variance(host, i, n):
            if not isinstance(host, dict):
                return np.ascontiguousarray(host[i, :n], np.float32)
            return {k: np.float32(host[k][i]) if k in ("mean", "std") else np.ascontiguousarray(host[k][i, :n], np.float32)
                    for k in ("signal", "original_signal", "spectrogram", "mean", "std")}  # CWT.decompose's keys, in its order
        items = []
        for i, d in enumerate(durs):
            n = {"frame": totals[i], "phone": len(d)}
            items.append({"mel": mel[i, :totals[i]].copy(), "duration": d,
                          "variances": {v: variance(var_host[v], i, n[lv]) for v, lv in zip(variances, levels)},
                          "priors": {p: float(prior_host[p][i]) for p in priors},
                          "silence_mask": frame_sil[i], "unexpanded_silence_mask": sils[i]})
        return items
