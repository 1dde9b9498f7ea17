"""Mel forward -> vocoder, the core of the reference's ``SpeechGenerator.generate_samples``
(litfass/synthesis/generator.py:151-223).  Of its optional post-processing, the audio augmentations that are well-defined
array operations - the resample, a room impulse response, Gaussian noise at an SNR (generate.py:82-104, generator.py:181,197-201) -
run on the device on the packed waveform (``augmentations=``, augment.py); VoiceFixer, ``PitchShift`` and the room simulation
itself (geometry -> impulse response) stay off-path.

The reference loops over utterances on the host: ``mel = result["mel"][i][~result["tgt_mask"][i]]``
goes to the CPU and back, one ``Synthesiser`` call each (generator.py:163-170).  Here the padded mel
batch never leaves HBM: the generator takes ``(B, T, 80)`` plus the valid frame counts and
synthesises every utterance from its own frames only (zero padding at ITS ends in every layer), which
is what the per-utterance loop computes.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch

from .fastdiff import FastDiff
from .hifigan import HifiGan
from .model import FastSpeech2, ForwardPipeline

INT16_MAX = float(np.iinfo(np.int16).max)


def int16_samples_to_float32(y: np.ndarray) -> np.ndarray:
    """generator.py:24-33."""
    if y.dtype == np.float32:
        return y
    if y.dtype != np.int16:
        raise ValueError(f"input samples not int16 or float32, but {y.dtype}")
    return y.astype(np.float32) / INT16_MAX


class SpeechGenerator:
    """``generate_samples(batch)`` -> ``{"fs", "audios"[, "durations"]}`` like the reference's
    (generator.py:151-223): ``audios`` is a list of float32 arrays, one per utterance, each the
    int16-quantised generator output rescaled by 1/32767 exactly as the reference does
    (Synthesiser.__call__ then int16_samples_to_float32).  Either object carries its own precision: the reference's mel and the
    reference's waveform at 16-bit speed are ``FastSpeech2(precision="mixed16")`` with ``HifiGan(precision="fp16")``.

    ``vocoder`` may be a ``FastDiff`` instead (the reference's ``SpeechGenerator(fastdiff=True)``, generator.py:48-57, 166-168:
    ``model.fastdiff_model.inference(mel, N=4)``): ``audios`` are then the float32 samples themselves, UNQUANTISED
    (int16_samples_to_float32 passes a float32 tensor through), drawn from torch's CPU generator utterance after utterance as the
    reference draws them; ``audio_dtype="int16"`` is refused.  The reference adds ``fastdiff_var`` to the mel first
    (generator.py:167); the engine does not expose it, so this is the mel alone."""

    def __init__(self, model: FastSpeech2, vocoder: "HifiGan | FastDiff", g2p_model=None, augmentations=None):
        """``augmentations``: a ``DeviceAugment`` (augment.py) applied to the float32 packed waveform on the device, between the
        vocoder and the copy to the host - to the int16-quantised samples rescaled, as the reference augments them, or to FastDiff's
        unquantised samples.  ``"fs"`` of a result is then the chain's final rate; ``audio_dtype="int16"`` is refused.  None (the
        default) leaves every path as it is without."""
        self.model, self.synth, self.g2p, self.augmentations = model, vocoder, g2p_model, augmentations
        self.model.eval()

    @property
    def fs(self) -> int:
        """the rate of the audio handed back"""
        fs = self.model.hparams.sampling_rate
        return fs if self.augmentations is None else self.augmentations.out_fs(fs)

    def _check_dtype(self, audio_dtype: str):
        if self.augmentations is not None and audio_dtype == "int16":
            raise ValueError("audio_dtype='int16' cannot be combined with augmentations: they run on the float32 samples")

    def _synthesize(self, result, audio_dtype: str):
        """vocoder + packing (+ augmentation) on the current stream -> (packed, offsets), device tensors"""
        packed, offsets = self.synth.synthesize_packed(result["mel"], self._lengths(result), audio_dtype)
        if self.augmentations is not None:
            max_len = result["mel"].shape[1] * self.synth.hop  # the host knows the padded frame count only
            packed, offsets, _ = self.augmentations(packed, offsets, self.model.hparams.sampling_rate, max_len)
        return packed, offsets

    def generate_from_text(self, text: str, speaker) -> np.ndarray:
        """generator.py:96-150 for the default (no priors) d-vector model: text -> phones the model
        knows -> batch of one -> audio.  ``speaker`` is a key of ``model.speaker2dvector`` or a
        256-d vector (the reference draws a random speaker when none is given; here it is explicit)."""
        from .frontend import text_to_batch
        if self.g2p is None:
            raise RuntimeError("no G2P model was given to SpeechGenerator")
        dvec = self.model.speaker2dvector[speaker] if not hasattr(speaker, "__len__") or isinstance(speaker, str) else speaker
        batch = text_to_batch(self.model.phone2id, self.g2p, text, dvec)
        return self.generate_samples(batch)["audios"][0]

    def _lengths(self, result) -> torch.Tensor:
        return (~result["tgt_mask"]).sum(dim=1).to(torch.int32)             # frames the reference keeps, :163 - stays on the device

    def _pinned(self, nbytes: int) -> torch.Tensor:
        buf = getattr(self, "_host", None)
        if buf is None or buf.numel() < nbytes:
            buf = self._host = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        return buf

    def generate_samples(self, batch: Dict, return_duration: bool = False, audio_dtype: str = "float32") -> Dict:
        """``audio_dtype="int16"`` hands back the int16 samples themselves (what ``Synthesiser.__call__`` returns in the reference, before
        int16_samples_to_float32); the default is the reference's float32."""
        if audio_dtype not in ("float32", "int16"):
            raise ValueError(f"audio_dtype must be 'float32' or 'int16', got {audio_dtype!r}")
        self._check_dtype(audio_dtype)
        result = self.model(batch, inference=True)                       # generator.py:158
        # float -> int16 (numpy's cast as Synthesiser.__call__ does it, __init__.py:39-43: truncation, tanh's +1.0 wraps to -32768),
        # the rescale by 1/32767 and the removal of the pads run on the device (fs2_op_wav_pack): one packed buffer comes across
        packed, offsets = self._synthesize(result, audio_dtype)
        off = offsets.cpu().numpy()                                      # waits for the generator; 8 (B + 1) bytes
        n = int(off[-1])
        host = self._pinned(n * packed.element_size())[:n * packed.element_size()].view(packed.dtype)
        host.copy_(packed[:n], non_blocking=True)
        torch.cuda.current_stream(packed.device).synchronize()
        flat = host.numpy()
        audios: List[np.ndarray] = [flat[off[b]:off[b + 1]].copy() for b in range(len(off) - 1)]  # owned: the staging buffer is reused
        out = {"fs": self.fs, "audios": audios}
        if return_duration:
            out["durations"] = [d.cpu() for d in result["duration_rounded"]]
        return out

    def pipeline(self, in_flight: int = 2, audio_dtype: str = "float32", return_duration: bool = False) -> "SpeechPipeline":
        return SpeechPipeline(self, in_flight, audio_dtype, return_duration)


class SpeechPipeline:
    """``generate_samples`` as a pipeline: while batch i's generator runs, batch i + 1's mel forward is queued beside it and batch
    i - 1's packed waveform crosses PCIe; the calling thread only slices.

        pipe = generator.pipeline(2)
        for batch in batches:
            for out in pipe.submit(batch):   # results come back in submission order, a batch or two later
                use(out)
        for out in pipe.drain():
            use(out)
        pipe.close()

    Each result is the dict ``generate_samples(batch, return_duration, audio_dtype)`` returns, bit for bit.  Stages:
      - the mel forward on a ``ForwardPipeline`` (``in_flight`` engine replicas, a stream and a thread each);
      - generator + fs2_op_wav_pack (+ the generator's ``augmentations``) on ONE vocoder stream driven by ONE thread: the fs2_vocoder handle has no clone and must not be
        entered concurrently.  The frame counts go from the forward's mask to the generator on the device;
      - the packed buffer (capacity ``B*T*hop``, or the augmentation chain's worst case: the total is known on the device only) and its offsets to pinned memory on one copy
        stream behind an event, queued by a copier thread (a small copy blocks its caller until the stream reaches it);
      - slicing by the offsets on the calling thread, once the copy has landed.
    The GPU never waits for the host's finishing; the host reads the forward's frame count T (as ever) and the landed offsets.

    ``audios`` are views of a pinned ring slot (``2 * in_flight + 2`` slots, up to ``in_flight + 1`` results pending): a result stays
    valid for the next ``in_flight`` calls of ``submit`` after it was handed over (copy it or consume it before) - the rule of
    ``ForwardPipeline``'s ``host_outputs``.  No graphs; in_flight + 2 streams."""

    def __init__(self, gen: SpeechGenerator, in_flight: int = 2, audio_dtype: str = "float32", return_duration: bool = False):
        import concurrent.futures as cf
        from .hifigan import _WAV_KINDS
        if in_flight < 1:
            raise ValueError("in_flight >= 1")
        if audio_dtype not in _WAV_KINDS:
            raise ValueError(f"audio_dtype must be one of {sorted(_WAV_KINDS)}, got {audio_dtype!r}")
        gen._check_dtype(audio_dtype)
        self.gen, self.audio_dtype, self.return_duration = gen, audio_dtype, return_duration
        self.device = gen.synth.device
        self.fwd = ForwardPipeline(gen.model, in_flight)
        self.voc_stream = torch.cuda.Stream(self.device)
        self.copy_stream = torch.cuda.Stream(self.device)
        self.voc_pool = cf.ThreadPoolExecutor(max_workers=1)
        self.copy_pool = cf.ThreadPoolExecutor(max_workers=1)
        self.window = in_flight + 1
        self._ring = [{} for _ in range(2 * in_flight + 2)]  # slot -> {"audio" / "offsets": flat pinned uint8 buffer}
        self.pending = []  # futures in submission order
        self.n = 0

    def _vocode(self, fwd_future, slot):
        out, fwd_done = fwd_future.result()
        vs = self.voc_stream
        with torch.cuda.device(self.device), torch.cuda.stream(vs):
            vs.wait_event(fwd_done)
            ForwardPipeline._record(out, vs)  # allocated on the forward's stream, read here
            packed, offsets = self.gen._synthesize(out, self.audio_dtype)  # one thread: an augmentation draws in submission order
            done = torch.cuda.Event()
            done.record(vs)
        return self.copy_pool.submit(self._to_host, out, fwd_done, packed, offsets, done, slot)

    @staticmethod
    def _slot_buffer(slot, key, like):
        nbytes = like.numel() * like.element_size()
        buf = slot.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = slot[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        return buf[:nbytes].view(like.dtype)

    def _to_host(self, out, fwd_done, packed, offsets, voc_done, slot):
        cs = self.copy_stream
        with torch.cuda.device(self.device), torch.cuda.stream(cs):
            cs.wait_event(voc_done)
            host, host_off = self._slot_buffer(slot, "audio", packed), self._slot_buffer(slot, "offsets", offsets)
            host.copy_(packed, non_blocking=True)
            host_off.copy_(offsets, non_blocking=True)
            packed.record_stream(cs)  # allocated on the vocoder stream, which goes on to the next batch
            offsets.record_stream(cs)
            done = torch.cuda.Event()
            done.record(cs)
        return out, fwd_done, host, host_off, done

    def _finished(self, fut) -> bool:
        if not fut.done() or not fut.result().done():
            return False
        return fut.result().result()[4].query()

    def _hand_over(self, fut) -> Dict:
        out, fwd_done, host, host_off, done = fut.result().result()
        done.synchronize()  # the copy has landed
        off, flat = host_off.numpy(), host.numpy()
        res = {"fs": self.gen.fs, "audios": [flat[off[b]:off[b + 1]] for b in range(len(off) - 1)]}
        if self.return_duration:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(fwd_done)
            ForwardPipeline._record(out["duration_rounded"], cur)
            res["durations"] = [d.cpu() for d in out["duration_rounded"]]
        return res

    def submit(self, batch) -> List[Dict]:
        """Queue one batch; returns the list (possibly empty) of finished-in-order results that fall out of the window."""
        slot = self._ring[self.n % len(self._ring)]
        self.n += 1
        self.pending.append(self.voc_pool.submit(self._vocode, self.fwd._start(batch), slot))
        outs = []
        while len(self.pending) > self.window:             # never more than the window behind: the host waits for the oldest
            outs.append(self._hand_over(self.pending.pop(0)))
        while self.pending and self._finished(self.pending[0]):  # and whatever has landed in the meantime
            outs.append(self._hand_over(self.pending.pop(0)))
        return outs

    def drain(self) -> List[Dict]:
        outs = [self._hand_over(f) for f in self.pending]
        self.pending = []
        return outs

    def close(self):
        self.drain()
        self.voc_pool.shutdown(wait=True)
        self.copy_pool.shutdown(wait=True)
        self.fwd.close()
