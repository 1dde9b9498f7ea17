"""The teacher-target helper (tests/_teacher.py) on the CPU oracle alone: feeding the oracle its own free-running decisions as
teacher targets reproduces its free-running forward bit for bit, so a GPU output fed the same way puts the oracle under the
GPU's decisions and nothing else (tests/test_gpu_graphs.py)."""
import pytest
import torch

from _teacher import teacher_targets
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
from oracle import oracle_cpu

PRIOR_STATS = {"pitch": {"min": -2.0, "max": 2.5, "mean": 0.1, "std": 1.5}, "energy": {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0},
               "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0}, "pitch_prior": {"min": -1.0, "max": 1.0},
               "duration_prior": {"min": 0.0, "max": 5.0}}


def _small(**kw):
    base = dict(n_phones=30, encoder_hidden=64, decoder_hidden=64, encoder_head=2, decoder_head=2, encoder_layers=1, decoder_layers=1,
                encoder_kernel_sizes=[5], decoder_kernel_sizes=[5], encoder_conv_filter_size=128, decoder_conv_filter_size=128,
                variance_filter_size=64, variance_nlayers=[2, 2, 2], variance_nbins=32, duration_filter_size=64)
    return Fs2Config(**{**base, **kw})


CASES = {
    "frame": (_small(), 1.2),
    "phone1": (_small(variance_levels=["phone", "frame", "frame"]), 1.2),
    "phone2_dw": (_small(variance_levels=["phone", "frame", "phone"], encoder_depthwise_conv=True, variance_depthwise_conv=True), 1.1),
    "phone3": (_small(variance_levels=["phone", "phone", "phone"], encoder_depthwise_conv=False, variance_depthwise_conv=False), 1.3),
    "priors_phone1": (_small(variance_levels=["phone", "frame", "frame"], priors=["pitch", "duration"], stats=PRIOR_STATS), 1.2),
    "guard": (_small(variance_levels=["frame", "phone", "frame"]), 0.3),  # the zero-duration guard fires: its durations are decisions too
}


def _flat(d):
    return {k: v for k, v in d.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_under_its_own_decisions_reproduces_itself(case):
    cfg, bias = CASES[case]
    sd = synth_state_dict(cfg, 4, randomize_norm=True, duration_bias=bias)
    inp = synth_inputs(cfg, 4, 23, seed=8, lengths=[23, 14, 1, 9])
    pri = {k: v for k, v in inp.items() if k.startswith("priors_")}
    free = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"], priors=pri, return_intermediates=True)
    if case == "guard":
        assert free["_zero_duration_guard"], "the guard case must exercise the guard"
    tgt = teacher_targets(cfg, free)
    forced = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"], priors=pri, teacher_targets=tgt, return_intermediates=True)
    a, b = _flat(free), _flat(forced)
    assert set(a) == set(b)
    for k in a:
        if k == "duration_rounded":
            assert torch.equal(a[k].long(), b[k].long())
        else:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for v in cfg.variances:  # the decisions themselves, not only what they led to
        assert torch.equal(free["_intermediates"][f"bucket_{v}"], forced["_intermediates"][f"bucket_{v}"]), v


def test_cwt_variances_are_refused():
    cfg = _small(variance_transforms=["cwt", "none", "none"],
                 stats={"pitch": {"min": 0.2, "max": 5.0, "mean": 0.1, "std": 1.5}, "energy": {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0},
                        "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0}})
    with pytest.raises(ValueError, match="CWT"):
        teacher_targets(cfg, {})
