"""MI355X-native FastSpeech2 / LightSpeech mel forward (drop-in for litfass.fastspeech2 forward)."""
from .config import Fs2Config, preset  # noqa: F401
from .weights import state_dict_spec, synth_state_dict, synth_inputs  # noqa: F401

__all__ = ["Fs2Config", "preset", "state_dict_spec", "synth_state_dict", "synth_inputs", "FastSpeech2", "Trainer", "MelAnalyzer",
           "slaney_mel_basis", "finish_contour", "masked_row_mean", "cwt_decompose", "FastDiff", "FastDiffConfig", "DeviceAugment", "Resample", "RoomImpulse",
           "GaussianSNR"]


def __getattr__(name):
    # the engine needs the HIP library; keep config/weights importable without it
    if name == "FastSpeech2":
        from .model import FastSpeech2
        return FastSpeech2
    if name == "Trainer":  # the training step: forward tape + backward + clip + AdamW / Noam
        from .training import Trainer
        return Trainer
    if name in ("FastDiff", "FastDiffConfig"):  # the FastDiff vocoder at inference (fs2_fd_*)
        from . import fastdiff
        return getattr(fastdiff, name)
    # the analysis front end: waveform -> log-mel + energy + training targets on the device
    if name in ("MelAnalyzer", "slaney_mel_basis", "finish_contour", "masked_row_mean", "cwt_decompose"):
        from . import analysis
        return getattr(analysis, name)
    # augmentation of the packed waveform on the device: resample, impulse response, noise at an SNR
    if name in ("DeviceAugment", "Resample", "RoomImpulse", "GaussianSNR"):
        from . import augment
        return getattr(augment, name)
    raise AttributeError(name)
