"""`generator_16bit`: a plain-torch CPU model of a HiFi-GAN generator that STORES its tensors in a 16-bit type - the yardstick the
precision="fp16" tests hold the engine's generator to (what tests/_f16.decoder_16bit is to the mixed16 decoder).

It restates oracle/hifigan_cpu.generator and passes through `_f16.rnd16(., tdt)` exactly the tensors vocoder_engine.hip stores, as
the engine stores them under fs2_op_set_vocoder_fused_resblock(1), the default:

  * every conv / transposed-conv weight, rounded once (fs2_voc_finalize); biases stay fp32;
  * the mel, at conv_pre's slab fill; conv_pre's output (stage 0) is stored RAW;
  * a conv that reads a raw stream stages lrelu(x) rounded again (the slab holds the activated operand);
  * the upsampler's output: ACTIVATED - rnd(lrelu(acc)) - when every resblock of the stage runs on LDS-resident tiles
    (32 / 64 / 128 channels where voc_resblock_mi16 takes the whole block or each of its pairs), RAW otherwise (the 256-channel
    stage of V1 and anything wider);
  * conv by conv (non-resident): c1's output ACTIVATED (c2 stages it untouched), c2's output + residual RAW;
  * LDS-resident pairs / blocks: slab X = the activated stream, slab Y = rnd(lrelu(c1)), both in the storage type; the raw
    residual is recovered from X as (a < 0 ? a / slope : a) in fp32 and only the sum is stored - ACTIVATED into X (inside a block)
    or to memory between two resident pair launches, RAW after the last pair of a block;
  * the stage accumulation: stage = rnd(r_0 / n), then rnd(stage + r_j / n) per further resblock; stored RAW (the stage outputs
    `debug_stage` returns);
  * conv_post stages rnd(lrelu(x, 0.01)); accumulation, bias, tanh and the wav are fp32.

Accumulation is fp32 everywhere (torch's conv1d on fp32 tensors holding 16-bit values).  Parameterised by torch.float32 /
torch.bfloat16 / torch.float16: with float32 nothing is rounded, the residual is carried instead of recovered and the stage mean
is the oracle's (sum) / n, so the model IS the oracle, bit for bit (tests/test_hifigan_fp16_cpu.py).  `knob` = any other value of
fs2_op_set_vocoder_fused_resblock models that launch form: 0 conv by conv everywhere, 9 resident tiles with raw streams between
launches, 2 / 4 / 7 / 50..100 another set of resident pairs and blocks (`resident_form`) and with it other streams stored activated.
Per-utterance zero padding follows hifigan_cpu.synthesize: every utterance runs alone on its first lengths[b] frames."""
import numpy as np
import torch
import torch.nn.functional as F

from _f16 import rnd16

SLOPE = 0.1


def _rb_geom(C, taps, dils, nw, mi16):
    c = (taps - 1) // 2
    dmax, dsum = max([1] + list(dils)), sum(d + 1 for d in dils)
    return (nw // (C // 32)) * mi16 * 16, c * (dsum - dils[0]), c * dmax


def _rb_lds(C, taps, dils, nw, mi16, esz):
    R, _, G = _rb_geom(C, taps, dils, nw, mi16)
    return ((R + 2 * G) + (R + 2 * ((taps - 1) // 2))) * C * esz


def resident_form(C, taps, dils, knob=1, esz=2):
    """voc_resblock_mi16 (vocoder_resblock.hip) restated: the form - 408 / 808 / 804 = 100 * waves + 16-row fragments per wave - this
    block (3 dilations) / pair (1) runs in on LDS tiles, 0 = conv by conv.  knob: fs2_op_set_vocoder_fused_resblock's values (0 off,
    1 default, 2 pairs only, 4 no 4-wave form, 7 whole blocks whatever taps * C, 9 = 1 here, 50..100 = the 4-wave form's threshold in
    percent); esz: bytes per stored element.  tests/test_voc_forms_cpu.py holds it to the library's own picker."""
    if not knob or (knob == 2 and len(dils) != 1) or C not in (32, 64, 128) or not taps & 1 or len(dils) not in (1, 3):
        return 0
    if len(dils) == 3 and taps * C > 224 and knob != 7:
        return 0
    if knob != 4:
        R, H, _ = _rb_geom(C, taps, dils, 4, 8)
        if _rb_lds(C, taps, dils, 4, 8, esz) <= 76 * 1024 and (R - 2 * H) * 100 >= R * (knob if knob >= 50 else 85):
            return 408
    for mi in (8, 4):
        R, H, _ = _rb_geom(C, taps, dils, 8, mi)
        if _rb_lds(C, taps, dils, 8, mi, esz) <= 150 * 1024 and (R - 2 * H) * 5 >= R * 4:
            return 800 + mi
    return 0


def resident(C, taps, dils, knob=1, esz=2):
    """does this block (3 dilations) / pair (1) run on LDS tiles?"""
    return resident_form(C, taps, dils, knob, esz) != 0


class _Stream:
    """A stored (1, C, T) tensor: `raw` and / or `act` = lrelu(raw), whichever the engine keeps (both in the float32 model)."""
    def __init__(self, raw=None, act=None):
        self.raw, self.act = raw, act


def generator_16bit(sd, cfg, mel, lengths, tdt, return_stages=False, knob=1):
    """mel (B, T, n_mels), lengths (B) or None -> wav (B, T * hop) fp32, zeros past each utterance (and per-utterance stage
    outputs, time-major), like hifigan_cpu.synthesize."""
    from oracle.hifigan_cpu import _t
    exact = tdt == torch.float32
    r = lambda t: rnd16(t, tdt)
    w = lambda n: r(_t(sd, n + ".weight"))
    b = lambda n: _t(sd, n + ".bias")
    inv_slope = float(torch.tensor(1.0) / torch.tensor(SLOPE))   # the kernel's 1.0f / slope
    nk = len(cfg.resblock_kernel_sizes)
    inv_n = float(torch.tensor(1.0) / torch.tensor(float(nk)))
    ch = cfg.channels()

    def store_raw(v):
        return _Stream(raw=r(v))

    def store_act(v):
        return _Stream(raw=v if exact else None, act=r(F.leaky_relu(v, SLOPE)))

    def operand(s):          # what a conv behind LeakyReLU(0.1) multiplies
        return s.act if s.act is not None else r(F.leaky_relu(s.raw, SLOPE))

    def residual_lds(s):     # a resident launch recovers the raw stream from its slab X
        if exact:
            return s.raw
        a = operand(s)
        return torch.where(a < 0, a * inv_slope, a)

    def pair(s, pfx, m, k, d, on_lds):
        """fp32 x + c2(lrelu(c1(lrelu(x)))) of one pair, before it is stored"""
        y = F.conv1d(operand(s), w(f"{pfx}.convs1.{m}"), b(f"{pfx}.convs1.{m}"), dilation=d, padding=(k * d - d) // 2)
        y = r(F.leaky_relu(y, SLOPE))
        y = F.conv1d(y, w(f"{pfx}.convs2.{m}"), b(f"{pfx}.convs2.{m}"), dilation=1, padding=(k - 1) // 2)
        return y + (residual_lds(s) if on_lds else s.raw)

    def one(mel_ct):
        stages = []
        x = r(F.conv1d(r(mel_ct), w("conv_pre"), b("conv_pre"), padding=3))
        stages.append(x)
        for i, (u, uk) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
            C = ch[i + 1]
            blocks = list(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes))
            whole = [resident(C, k, list(ds), knob) for k, ds in blocks]
            pairs = [[resident(C, k, [d], knob) for d in ds] for k, ds in blocks]
            stage_act = knob != 9 and all(wh or all(pr) for wh, pr in zip(whole, pairs))
            acc = F.conv_transpose1d(r(F.leaky_relu(x, SLOPE)), w(f"ups.{i}"), b(f"ups.{i}"), stride=u, padding=(uk - u) // 2)
            up = store_act(acc) if stage_act else store_raw(acc)
            xs = None
            for j, (k, ds) in enumerate(blocks):
                pfx, s = f"resblocks.{i * nk + j}", up
                for m, d in enumerate(ds):
                    if whole[j]:
                        on_lds, act_out = True, m < 2
                    else:
                        on_lds = pairs[j][m]
                        act_out = m < 2 and pairs[j][m] and pairs[j][m + 1] and knob != 9
                    v = pair(s, pfx, m, k, d, on_lds)
                    if m < 2:
                        s = store_act(v) if act_out else store_raw(v)
                if exact:
                    xs = v if xs is None else xs + v
                else:
                    xs = r(v * inv_n) if xs is None else r(xs + v * inv_n)
            x = xs / nk if exact else xs
            stages.append(x)
        x = r(F.leaky_relu(x))   # default slope 0.01
        x = torch.tanh(F.conv1d(x, w("conv_post"), b("conv_post"), padding=3))
        return x, stages

    mel = torch.as_tensor(mel, dtype=torch.float32)
    B, T, _ = mel.shape
    hop = int(np.prod(cfg.upsample_rates))
    wav = torch.zeros(B, T * hop)
    all_stages = []
    with torch.no_grad():
        for u in range(B):
            n = T if lengths is None else int(lengths[u])
            if n == 0:
                all_stages.append([])
                continue
            y, st = one(mel[u, :n].T.unsqueeze(0))
            wav[u, :n * hop] = y[0, 0]
            all_stages.append([s[0].T.contiguous() for s in st])
    return (wav, all_stages) if return_stages else wav


def errs(a, b):
    """(max, mean) of |a - b|"""
    d = (a - b).abs()
    return float(d.max()), float(d.mean())


# ---- shared inputs of the precision="fp16" tests -----------------------------------------------------------------------------------
def two_stage_cfg():
    from lightningfastspeech2_amd.hifigan import HifiGanConfig
    return HifiGanConfig(upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=128,
                         resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 2, 3], [1, 3, 5]])


def random_mel(seed, B, T):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal((B, T, 80)) * 1.5 - 4.0).astype(np.float32))


def saturation_case():
    """(cfg, plain weights, scaled weights, mel (1, 45, 80)): conv_pre x 1e4 drives stage 0 beyond binary16's range; both
    upsamplers / 100 bring the later stages back (LeakyReLU is positively homogeneous), and no weight tensor is pushed into
    binary16's subnormal range."""
    from lightningfastspeech2_amd.hifigan import synth_state_dict
    cfg = two_stage_cfg()
    sd = synth_state_dict(cfg, 4)
    big = dict(sd)
    big["conv_pre.weight"] = sd["conv_pre.weight"] * np.float32(1e4)
    big["conv_pre.bias"] = sd["conv_pre.bias"] * np.float32(1e4)
    big["ups.0.weight"] = sd["ups.0.weight"] / np.float32(100)
    big["ups.1.weight"] = sd["ups.1.weight"] / np.float32(100)
    return cfg, sd, big, random_mel(9, 1, 45)
