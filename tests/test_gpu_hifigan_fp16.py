"""HifiGan(precision="fp16") on the device: the generator with every stored tensor in IEEE binary16 (FS2_F16).

Errors are measured against the reference fixtures or the fp32 oracle, never against the code under test, and the bars are not
fixed numbers: on the same input every test computes the errors `yb` / `yh` of the CPU model of a 16-bit-storage generator
(tests/_voc16.generator_16bit with bfloat16 / float16) and the errors `gb` / `gh` of the engine in "bf16" / "fp16", each as
(max, mean) of |x - reference|, and asserts
  (a) calibration     yb / 2 <= gb <= 2 yb      the model describes the engine
  (b) against the model     gh <= 2 yh
  (c) against bf16          gh <= gb / 4        (unit roundoffs differ by 8; the model's own ratio is 6.6 - 8.2)
  (d) everything is finite.
Every measured tuple goes to the parity report (test names vocoder_fp16_*)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import _voc16
from _f16 import F16_MAX
from test_gpu_forward import _report
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.hifigan import HifiGan, HifiGanConfig, Synthesiser, _config_to_c, synth_state_dict
from oracle import hifigan_cpu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BF, H = torch.bfloat16, torch.float16


def _valid(x, lengths, per_frame):
    """the valid rows of every utterance, concatenated: x = (B, S[, C]) tensor or a list of per-utterance tensors"""
    return torch.cat([x[b][:int(n) * per_frame].reshape(-1) for b, n in enumerate(lengths)])


def _check(test, case, ref, yb, yh, gb, gh, scale=1.0, calibrate=True, vs_bf16=True):
    """ref and the four candidates: flat tensors over the same entries -> asserts (a) - (d), reports the tuples"""
    assert all(bool(torch.isfinite(t).all()) for t in (yb, yh, gb, gh)), (test, case)                      # (d)
    e = {k: _voc16.errs(v, ref) for k, v in (("yb", yb), ("yh", yh), ("gb", gb), ("gh", gh))}
    _report(test=test, case=case, scale=scale, **{k: [v[0] / scale, v[1] / scale] for k, v in e.items()})
    for i, what in enumerate(("max", "mean")):
        if calibrate:
            assert e["yb"][i] / 2 <= e["gb"][i] <= 2 * e["yb"][i], (test, case, what, "calibration", e)   # (a)
        assert e["gh"][i] <= 2 * e["yh"][i], (test, case, what, "fp16 vs model", e)                        # (b)
        if vs_bf16:
            assert e["gh"][i] <= e["gb"][i] / 4, (test, case, what, "fp16 vs bf16", e)                     # (c)
    return e


def _fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = HifiGanConfig.from_json(str(z["config"]))
    return z, cfg, synth_state_dict(cfg, int(z["seed"]))


@functools.lru_cache(maxsize=None)
def _seam():
    """the input of test_stage_outputs_and_tile_seams, the oracle's answer and both models' (computed once)"""
    cfg = HifiGanConfig()
    sd = synth_state_dict(cfg, 5)
    mel, lengths = _voc16.random_mel(9, 3, 45), torch.tensor([45, 29, 1], dtype=torch.int32)
    ref = hifigan_cpu.synthesize(sd, cfg, mel, lengths, return_stages=True)
    mb = _voc16.generator_16bit(sd, cfg, mel, lengths, BF, return_stages=True)
    mh = _voc16.generator_16bit(sd, cfg, mel, lengths, H, return_stages=True)
    return cfg, sd, mel, lengths, ref, mb, mh


@pytest.mark.parametrize("name", ["hifigan_two_stage", "hifigan_v1"])
def test_fixtures(name):
    z, cfg, sd = _fixture(name)
    mel, lengths = torch.from_numpy(z["mel"]), torch.from_numpy(z["lengths"])
    L = lengths.tolist()
    ref = torch.cat([torch.from_numpy(z[f"wav_{b}"]) for b in range(len(L))])
    yb = _valid(_voc16.generator_16bit(sd, cfg, mel, lengths, BF), L, cfg.hop)
    yh = _valid(_voc16.generator_16bit(sd, cfg, mel, lengths, H), L, cfg.hop)
    g = HifiGan(cfg, sd, precision="fp16")
    wav = g.synthesize(mel, lengths).cpu()
    gb = _valid(HifiGan(cfg, sd, precision="bf16").synthesize(mel, lengths).cpu(), L, cfg.hop)
    _check("vocoder_fp16_fixture", name, ref, yb, yh, gb, _valid(wav, L, cfg.hop))
    for b, n in enumerate(L):
        assert float(wav[b, n * cfg.hop:].abs().sum()) == 0.0
        alone = g.synthesize(mel[b:b + 1, :n]).cpu()
        assert torch.equal(alone[0], wav[b, :n * cfg.hop])


def test_stages_and_tile_seams():
    cfg, sd, mel, lengths, (ref_wav, ref_st), (mb_wav, mb_st), (mh_wav, mh_st) = _seam()
    L = lengths.tolist()
    gh, gb = HifiGan(cfg, sd, precision="fp16"), HifiGan(cfg, sd, precision="bf16")
    wav_h, wav_b = gh.synthesize(mel, lengths).cpu(), gb.synthesize(mel, lengths).cpu()
    for s in range(len(cfg.upsample_rates) + 1):
        up = int(np.prod(cfg.upsample_rates[:s])) if s else 1
        pick = lambda per_utt: torch.cat([per_utt[b][s].reshape(-1) for b in range(len(L))])
        ref = pick(ref_st)
        _check("vocoder_fp16_stage", f"seam_stage{s}", ref, pick(mb_st), pick(mh_st), _valid(gb.debug_stage(s).cpu(), L, up),
               _valid(gh.debug_stage(s).cpu(), L, up), scale=float(ref.abs().max()) + 1.0, calibrate=False)
    _check("vocoder_fp16_stage", "seam_wav", _valid(ref_wav, L, cfg.hop), _valid(mb_wav, L, cfg.hop), _valid(mh_wav, L, cfg.hop),
           _valid(wav_b, L, cfg.hop), _valid(wav_h, L, cfg.hop))


@pytest.mark.parametrize("seed,mel_seed,T,lengths", [(8, 2, 23, (23, 10)), (11, 4, 37, (37, 12, 1))])
def test_launch_forms_agree(seed, mel_seed, T, lengths):
    """knob 0 (conv by conv), 1 (resident tiles, activated streams: the default, what the model restates) and 9 (resident tiles,
    raw streams) each meet (b) against the oracle"""
    cfg = HifiGanConfig()
    sd = synth_state_dict(cfg, seed)
    L = list(lengths)
    mel, ln = _voc16.random_mel(mel_seed, len(L), T), torch.tensor(L, dtype=torch.int32)
    ref = _valid(hifigan_cpu.synthesize(sd, cfg, mel, ln), L, cfg.hop)
    yh = _voc16.errs(_valid(_voc16.generator_16bit(sd, cfg, mel, ln, H), L, cfg.hop), ref)
    g = HifiGan(cfg, sd, precision="fp16")
    got = {}
    try:
        for knob in (0, 1, 9):
            _lib.load().fs2_op_set_vocoder_fused_resblock(knob)
            got[knob] = g.synthesize(mel, ln).cpu()
    finally:
        _lib.load().fs2_op_set_vocoder_fused_resblock(1)
    for knob, wav in got.items():
        assert bool(torch.isfinite(wav).all())
        e = _voc16.errs(_valid(wav, L, cfg.hop), ref)
        own = _voc16.errs(_valid(_voc16.generator_16bit(sd, cfg, mel, ln, H, knob=knob), L, cfg.hop), ref)
        _report(test="vocoder_fp16_forms", case=f"seed{seed}_knob{knob}", gh=list(e), yh=list(yh), yh_this_form=list(own))
        assert e[0] <= 2 * yh[0] and e[1] <= 2 * yh[1], (knob, e, yh)


def test_saturation():
    """conv_pre x 1e4 stores large finite numbers: 7 % of stage 0 lies beyond +-65504 and must come back as +-65504, not as inf (which
    the next LeakyReLU / MFMA would turn into NaN); the wav must be the clamping model's, not merely finite."""
    cfg, sd, big, mel = _voc16.saturation_case()
    ref_plain = hifigan_cpu.synthesize(sd, cfg, mel)
    yh = _voc16.errs(_voc16.generator_16bit(sd, cfg, mel, None, H), ref_plain)
    ref, ref_st = hifigan_cpu.synthesize(big, cfg, mel, return_stages=True)
    frac = float((ref_st[0][0].abs() > F16_MAX).float().mean())
    model = _voc16.generator_16bit(big, cfg, mel, None, H)
    clamp = _voc16.errs(model, ref)
    assert 0.01 <= frac <= 0.5 and clamp[0] > 100 * yh[0], (frac, clamp, yh)
    g = HifiGan(cfg, big, precision="fp16")
    wav = g.synthesize(mel).cpu()
    stages = [g.debug_stage(s).cpu() for s in range(len(cfg.upsample_rates) + 1)]
    assert bool(torch.isfinite(wav).all()) and all(bool(torch.isfinite(s).all()) for s in stages)
    assert float(stages[0].abs().max()) <= F16_MAX
    e = _voc16.errs(wav, model)
    _report(test="vocoder_fp16_saturation", case="two_stage_x1e4", beyond_range=frac, stage0_max=float(stages[0].abs().max()),
            model_vs_oracle=list(clamp), engine_vs_model=list(e), bound=[2 * yh[0], 2 * yh[1]])
    assert e[0] <= 2 * yh[0] and e[1] <= 2 * yh[1], (e, yh)


def test_full_size_time_shift_equivariance():
    """test_gpu_hifigan.py's construction at the benchmark's utterance length, in fp16: dropping the first k frames shifts the
    waveform by k * 256 samples away from the edges, bit for bit"""
    cfg = HifiGanConfig()
    g = HifiGan(cfg, synth_state_dict(cfg, 21), precision="fp16")
    T, k, margin, hop = 1536, 8, 32, cfg.hop
    mel = _voc16.random_mel(4, 2, T)
    full = g.synthesize(mel).cpu()
    shifted = g.synthesize(mel[:, k:].contiguous()).cpu()
    assert bool(torch.isfinite(full).all()) and float(full.abs().max()) <= 1.0
    assert torch.equal(full[:, (k + margin) * hop:(T - margin) * hop], shifted[:, margin * hop:(T - k - margin) * hop])
    assert not torch.equal(full[:, :margin * hop // 2], shifted[:, :margin * hop // 2])
    _report(test="vocoder_fp16_shift", case=f"T{T}_k{k}", bit_exact=True)


@pytest.mark.parametrize("rates,kernels", [((4, 2), (8, 4)), ((4, 2), (12, 6)), ((2, 2), (2, 2)), ((8, 2), (16, 6))])
def test_transposed_conv_tap_windows(rates, kernels):
    cfg = HifiGanConfig(upsample_rates=list(rates), upsample_kernel_sizes=list(kernels), upsample_initial_channel=128,
                        resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]])
    sd = synth_state_dict(cfg, 11)
    L = [60, 37, 2]
    mel, lengths = _voc16.random_mel(3, 3, 60), torch.tensor(L, dtype=torch.int32)
    ref_wav, ref_st = hifigan_cpu.synthesize(sd, cfg, mel, lengths, return_stages=True)
    m_wav, m_st = _voc16.generator_16bit(sd, cfg, mel, lengths, H, return_stages=True)
    g = HifiGan(cfg, sd, precision="fp16")
    wav = g.synthesize(mel, lengths).cpu()
    assert bool(torch.isfinite(wav).all())
    case = f"r{rates[0]}x{rates[1]}_k{kernels[0]}x{kernels[1]}"
    for s in range(len(rates) + 2):
        if s <= len(rates):
            up = int(np.prod(rates[:s])) if s else 1
            pick = lambda per_utt: torch.cat([per_utt[b][s].reshape(-1) for b in range(3)])
            ref, yh, gh = pick(ref_st), pick(m_st), _valid(g.debug_stage(s).cpu(), L, up)
        else:
            ref, yh, gh = _valid(ref_wav, L, cfg.hop), _valid(m_wav, L, cfg.hop), _valid(wav, L, cfg.hop)
        ey, eg = _voc16.errs(yh, ref), _voc16.errs(gh, ref)
        _report(test="vocoder_fp16_taps", case=f"{case}_{'wav' if s > len(rates) else f'stage{s}'}", yh=list(ey), gh=list(eg))
        assert eg[0] <= 2 * ey[0] and eg[1] <= 2 * ey[1], (case, s, eg, ey)


def test_runtime_stride_build():
    cfg = HifiGanConfig(upsample_rates=[2, 2, 2], upsample_kernel_sizes=[4, 4, 4], upsample_initial_channel=1024,
                        resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]])
    sd = synth_state_dict(cfg, 4)
    L = [40, 23]
    mel, lengths = _voc16.random_mel(1, 2, 40), torch.tensor(L, dtype=torch.int32)
    ref = _valid(hifigan_cpu.synthesize(sd, cfg, mel, lengths), L, cfg.hop)
    ey = _voc16.errs(_valid(_voc16.generator_16bit(sd, cfg, mel, lengths, H), L, cfg.hop), ref)
    wav = HifiGan(cfg, sd, precision="fp16").synthesize(mel, lengths).cpu()
    assert bool(torch.isfinite(wav).all())
    eg = _voc16.errs(_valid(wav, L, cfg.hop), ref)
    _report(test="vocoder_fp16_wide", case="c1024", yh=list(ey), gh=list(eg))
    assert eg[0] <= 2 * ey[0] and eg[1] <= 2 * ey[1], (eg, ey)


def test_synthesiser_int16():
    z, cfg, sd = _fixture("hifigan_v1")
    ck = {}
    for k, w in sd.items():
        if k.endswith(".weight"):
            t = torch.from_numpy(w)
            ck[k[:-7] + ".weight_g"] = t.flatten(1).norm(dim=1).reshape(-1, *([1] * (t.ndim - 1)))
            ck[k[:-7] + ".weight_v"] = t.clone()
        else:
            ck[k] = torch.from_numpy(w)
    n = int(z["lengths"][0])
    mel = torch.from_numpy(z["mel"][0, :n])
    yh_max = _voc16.errs(_voc16.generator_16bit(sd, cfg, mel[None], None, H)[0], torch.from_numpy(z["wav_0"]))[0]
    out = Synthesiser(device="cuda:0", checkpoint={"generator": ck}, precision="fp16")(mel)
    assert out.dtype == np.int16 and out.shape == (1, n * 256)
    d = int(np.abs(out.astype(np.int32) - z["int16_0"].astype(np.int32)).max())
    bound = math.ceil(2 * yh_max * 32768) + 1
    _report(test="vocoder_fp16_int16", case="hifigan_v1", lsb=d, bound=bound, yh_max=yh_max)
    assert d <= bound, (d, bound)


@pytest.mark.parametrize("dtype", [_lib.FS2_MIXED, _lib.FS2_MIXED_X3, _lib.FS2_F32_X3, _lib.FS2_MIXED_F16_X3])
def test_create_refuses_engine_modes(dtype):
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.fs2_voc_create(C.byref(_config_to_c(HifiGanConfig(), dtype)), C.byref(h)) == _lib.FS2_ERR_ARG
    assert not h.value
    assert lib.fs2_voc_create(C.byref(_config_to_c(HifiGanConfig(), _lib.FS2_F16)), C.byref(h)) == _lib.FS2_OK and h.value
    lib.fs2_voc_destroy(h)


def test_phonemes_to_samples():
    """test_mel_forward_into_vocoder_...'s small model through SpeechGenerator.generate_samples: ("mixed16", "fp16") keeps the
    oracle's durations and is closer to the oracle's per-utterance audio than ("mixed3", "bf16")"""
    from lightningfastspeech2_amd.config import Fs2Config
    from lightningfastspeech2_amd.model import FastSpeech2
    from lightningfastspeech2_amd.synthesis import SpeechGenerator
    from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict as fs2_sd
    from oracle import oracle_cpu
    cfg = Fs2Config(n_phones=40, encoder_hidden=64, decoder_hidden=64, encoder_head=2, decoder_head=2,
                    encoder_layers=2, decoder_layers=2, encoder_kernel_sizes=[3, 5], decoder_kernel_sizes=[5, 3],
                    encoder_conv_filter_size=128, decoder_conv_filter_size=128, encoder_depthwise_conv=False,
                    decoder_depthwise_conv=False, variance_filter_size=64, variance_depthwise_conv=False,
                    variance_nlayers=[2, 2, 2], duration_filter_size=64, duration_depthwise_conv=False, n_mels=80)
    sd = fs2_sd(cfg, 3, randomize_norm=True, duration_bias=1.3)
    inp = synth_inputs(cfg, 3, 12, seed=5, lengths=[12, 8, 3])
    vcfg = _voc16.two_stage_cfg()
    vsd = synth_state_dict(vcfg, 4)
    ref = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"])
    batch = {"phones": torch.from_numpy(inp["phones"]), "speaker": torch.from_numpy(inp["speaker"])}
    want = []
    for b in range(3):
        keep = ~ref["tgt_mask"][b]
        wav = hifigan_cpu.synthesize(vsd, vcfg, ref["mel"][b][keep].unsqueeze(0))[0]
        want.append((wav.numpy() * 32768.0).astype("int16").astype(np.float32) / 32767.0)
    err = {}
    for front, back in (("mixed16", "fp16"), ("mixed3", "bf16")):
        gen = SpeechGenerator(FastSpeech2(cfg, sd, precision=front, device="cuda:0"), HifiGan(vcfg, vsd, precision=back))
        out = gen.generate_samples(batch, return_duration=True)
        assert out["fs"] == 22050 and len(out["audios"]) == 3
        e = 0.0
        for b in range(3):
            got = out["audios"][b]
            assert got.dtype == np.float32 and got.shape == want[b].shape
            assert torch.equal(out["durations"][b], ref["duration_rounded"][b])
            e = max(e, float(np.abs(got - want[b]).max()))
        err[back] = e
    _report(test="vocoder_fp16_pipeline", case="small_model", audio_max_mixed16_fp16=err["fp16"], audio_max_mixed3_bf16=err["bf16"])
    assert err["fp16"] < err["bf16"], err
