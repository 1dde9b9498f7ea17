"""CPU checks of the yardstick of HifiGan(precision="fp16"): tests/_voc16.generator_16bit, the plain-torch model of a generator
that stores its tensors in a 16-bit type.  (1) With float32 "storage" it IS the oracle, bit for bit, in all three launch forms.
(2) Its binary16 error against the reference fixtures is at most a quarter of its bf16 error: the unit roundoffs differ by 8, the
measured ratios are 6.6-8.2, so 4 leaves a factor of about 1.6.  (3) The inputs of the GPU saturation test are what that test
claims: stage 0 overflows binary16, the later stages do not, and clamping is visible far above the rounding error."""
import os

import numpy as np
import pytest
import torch

import _voc16
from _f16 import F16_MAX
from lightningfastspeech2_amd.hifigan import HifiGanConfig, synth_state_dict
from oracle import hifigan_cpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = HifiGanConfig.from_json(str(z["config"]))
    mel, lengths = torch.from_numpy(z["mel"]), torch.from_numpy(z["lengths"])
    wav = torch.zeros(mel.shape[0], mel.shape[1] * cfg.hop)
    for b, n in enumerate(lengths.tolist()):
        wav[b, :n * cfg.hop] = torch.from_numpy(z[f"wav_{b}"])
    return cfg, synth_state_dict(cfg, int(z["seed"])), mel, lengths, wav


def _seam():
    cfg = HifiGanConfig()
    return cfg, synth_state_dict(cfg, 5), _voc16.random_mel(9, 3, 45), torch.tensor([45, 29, 1], dtype=torch.int32)


@pytest.mark.parametrize("case", ["hifigan_two_stage", "seam"])
@pytest.mark.parametrize("knob", [1, 0, 9])
def test_float32_model_is_the_oracle(case, knob):
    cfg, sd, mel, lengths = _seam() if case == "seam" else _fixture(case)[:4]
    ref, ref_st = hifigan_cpu.synthesize(sd, cfg, mel, lengths, return_stages=True)
    wav, st = _voc16.generator_16bit(sd, cfg, mel, lengths, torch.float32, return_stages=True, knob=knob)
    assert torch.equal(wav, ref)
    for a, b in zip(st, ref_st):
        assert len(a) == len(b) == len(cfg.upsample_rates) + 1
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["hifigan_two_stage", "hifigan_v1"])
def test_binary16_model_is_four_times_closer_than_bf16(name):
    cfg, sd, mel, lengths, fix = _fixture(name)
    yb = _voc16.errs(_voc16.generator_16bit(sd, cfg, mel, lengths, torch.bfloat16), fix)
    yh = _voc16.errs(_voc16.generator_16bit(sd, cfg, mel, lengths, torch.float16), fix)
    print(name, "bf16 (max, mean)", yb, "binary16", yh, "ratio", yb[0] / yh[0], yb[1] / yh[1])
    assert yh[0] <= yb[0] / 4 and yh[1] <= yb[1] / 4, (yb, yh)
    assert yh[0] <= 1e-3   # under F32_TOL, the fp32 mode's bar (tests/test_gpu_hifigan.py)


def test_resident_decisions_of_the_v1_generator():
    """The port of voc_resblock_mi16: which V1 blocks run on LDS tiles, as vocoder_resblock.hip's comments state them."""
    d = [1, 3, 5]
    assert not _voc16.resident(256, 3, d) and not _voc16.resident(256, 3, [1])          # 256 channels: conv by conv
    assert _voc16.resident(32, 3, d) and _voc16.resident(32, 7, d) and _voc16.resident(64, 3, d)   # whole blocks
    assert not _voc16.resident(64, 7, d) and not _voc16.resident(32, 11, d)             # K loop too long: pair by pair
    assert all(_voc16.resident(C, k, [x]) for C in (32, 64) for k in (3, 7, 11) for x in d)
    assert not _voc16.resident(64, 3, d, knob=0)


def test_saturation_construction():
    cfg, sd, big, mel = _voc16.saturation_case()
    ref, ref_st = hifigan_cpu.synthesize(big, cfg, mel, return_stages=True)
    s0 = ref_st[0][0]
    frac = float((s0.abs() > F16_MAX).float().mean())
    assert 0.01 <= frac <= 0.5, frac
    for s in ref_st[0][1:]:
        assert float(s.abs().max()) < F16_MAX
    for n, w in big.items():   # no weight tensor in binary16's subnormal range: its typical entry is a normal number
        if n.endswith(".weight"):
            assert float(np.median(np.abs(w))) > 2.0 ** -14, n
    wav, st = _voc16.generator_16bit(big, cfg, mel, None, torch.float16, return_stages=True)
    assert torch.isfinite(wav).all() and all(torch.isfinite(s).all() for s in st[0])
    assert float(st[0][0].abs().max()) == F16_MAX
    plain = _voc16.errs(_voc16.generator_16bit(sd, cfg, mel, None, torch.float16), hifigan_cpu.synthesize(sd, cfg, mel))
    clamp = _voc16.errs(wav, ref)
    print("stage-0 entries beyond 65504:", frac, "clamping model vs oracle", clamp, "unscaled binary16 error", plain)
    assert clamp[0] > 100 * plain[0], (clamp, plain)
