"""Which kernel instantiations a HiFi-GAN generator launches: the walk of fs2_voc_synthesize (vocoder_engine.hip) restated on the
host, with both choices - the conv tile height and the resident-resblock form - asked of the library's own pickers
(fs2_op_vocoder_conv_tile, fs2_op_vocoder_resblock_form; no device needed).  tests/test_voc_forms_cpu.py enumerates the reachable
instantiations with it and pins them; tests/test_gpu_hifigan_forms.py holds the engine's own launch record to it, launch for launch.

A launch is spelt as lightningfastspeech2_amd.hifigan.decode_launch spells it:
  ("conv", precision, MI16, CP, in_fp32, post, shift)   /   ("resblock", precision, form, channels, npairs, out_act, x_act)
and an instantiation - what the tables hold - is a launch without the flags that are kernel arguments, not template arguments:
  ("conv", precision, MI16, CP)   /   ("resblock", precision, form, channels, npairs, out_act)
(npairs is an argument too, but a whole block and a pair walk the kernel differently, and MID exists for pairs only)."""
import contextlib
import ctypes as C

import torch

import _voc16
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.hifigan import HifiGanConfig, _PRECISIONS

DTYPES = ("fp32", "bf16", "fp16")
KNOBS = (0, 1, 2, 4, 7, 9, 60)               # fs2_op_set_vocoder_fused_resblock: every value with a meaning of its own, 60 for 50..100
LIMITS = (0, 150, 76, 52, 36, 24, 12)        # fs2_op_set_vocoder_lds_limit (KiB) of the GPU sweeps
CP_BUILDS = (32, 64, 128, 256, 512)          # compile-time channel strides of vocoder_conv_kernel; anything else runs CP = 0


def _cfg(initial, rates, kernels, ks, dils):
    return HifiGanConfig(upsample_rates=list(rates), upsample_kernel_sizes=list(kernels), upsample_initial_channel=initial,
                         resblock_kernel_sizes=list(ks), resblock_dilation_sizes=[list(d) for d in dils])


# name -> (config, weight seed, mel seed, mel frames, lengths): the smallest shapes that cross several tiles in every stage, ragged
CONFIGS = {
    "v1": (HifiGanConfig(), 5, 9, 45, (45, 29, 1)),                                    # test_gpu_hifigan_fp16._seam()'s input
    "wide": (_cfg(1024, (2, 2, 2), (4, 4, 4), (3,), ((1, 3, 5),)), 4, 1, 40, (40, 23)),
    "two_stage": (_voc16.two_stage_cfg(), 4, 2, 23, (23, 10)),
    "mid": (_cfg(256, (4, 2, 2), (8, 4, 4), (3, 7), ((1, 3, 5), (1, 3, 5))), 6, 3, 30, (30, 17, 1)),
    "long_dilation": (_cfg(256, (2,), (4,), (11,), ((1, 3, 9),)), 7, 5, 40, (40, 9)),
}


@contextlib.contextmanager
def knobs(knob, limit):
    """the calling thread's two vocoder knobs for the body, the defaults (1, 0) behind it"""
    lib = _lib.load()
    try:
        assert lib.fs2_op_set_vocoder_fused_resblock(knob) == _lib.FS2_OK and lib.fs2_op_set_vocoder_lds_limit(limit) == _lib.FS2_OK
        yield lib
    finally:
        lib.fs2_op_set_vocoder_fused_resblock(1)
        lib.fs2_op_set_vocoder_lds_limit(0)


def resblock_form(lib, precision, channels, taps, dils):
    d = (C.c_int32 * 3)(*dils)
    f = lib.fs2_op_vocoder_resblock_form(_PRECISIONS[precision], channels, taps, d, len(dils))
    assert f in (0, 408, 808, 804), f
    return f


def conv_tile(lib, precision, n, cin, taps, dil, shift, post):
    """(MI16, CP) of the conv kernel for this layer under the calling thread's LDS limit"""
    pad = C.c_int32(0)
    mi = lib.fs2_op_vocoder_conv_tile(_PRECISIONS[precision], n, cin, taps, dil, int(shift), int(post), C.byref(pad))
    assert mi in (14, 8, 4, 2), (mi, n, cin, taps, dil)
    return mi, pad.value if pad.value in CP_BUILDS else 0


def up_taps(k, s):
    """ConvTranspose1d(k, stride s, padding (k - s) / 2) as the conv up_layer (vocoder_engine.hip) packs: (taps, two tap windows?)"""
    p = (k - s) // 2
    ms = [m for f in range(s) for m in range(-k, k + 1) if 0 <= m * s + f + p < k]
    K, pad = max(ms) - min(ms) + 1, max(ms)
    jlo, jhi = [K] * s, [-1] * s
    for f in range(s):
        for j in range(K):
            if 0 <= (pad - j) * s + f + p < k:
                jlo[f], jhi[f] = min(jlo[f], j), max(jhi[f], j)
    fshift, two = s, K >= 2
    for f in range(s):
        if not two:
            break
        if jlo[f] > 1 or jhi[f] - (1 if jlo[f] >= 1 else 0) > K - 2:
            two = False
        if jlo[f] >= 1 and fshift == s:
            fshift = f
        if jlo[f] < 1 and fshift != s:
            two = False
    return (K - 1 if two else K), bool(two and fshift < s)


def layers(lib, cfg, precision, knob):
    """fs2_voc_synthesize's walk under resblock knob `knob` (which must be the calling thread's): the launches in order, a conv as
    ("conv", n, cin, taps, dil, shift, post, in_fp32) - its tile is the LDS limit's business, `plan` - and a resident launch as
    decode_launch spells it"""
    out, ch = [], cfg.channels()
    conv = lambda n, cin, taps, dil, shift=False, post=False, in_fp32=False: out.append(("conv", n, cin, taps, dil, shift, post, in_fp32))
    form = lambda c, k, ds: resblock_form(lib, precision, c, k, ds)
    blocks = list(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes))
    conv(ch[0], cfg.num_mels, 7, 1, in_fp32=True)
    for i, (u, uk) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        c = ch[i + 1]
        packed = c in (32, 64, 128)   # fs2_voc_finalize packs the six convs of a block back to back at these widths only
        stage_act = knob != 9 and packed and all(form(c, k, ds) or all(form(c, k, [d]) for d in ds) for k, ds in blocks)
        taps, shift = up_taps(uk, u)
        conv(u * c, ch[i], taps, 1, shift)
        for k, ds in blocks:
            whole = form(c, k, ds) if packed else 0
            if whole:
                out.append(("resblock", precision, whole, c, 3, False, stage_act))
                continue
            res = [form(c, k, [d]) if packed else 0 for d in ds]
            for m, d in enumerate(ds):
                if res[m]:
                    x_act = stage_act if m == 0 else bool(res[m - 1] and knob != 9)
                    out_act = bool(m < 2 and res[m + 1] and knob != 9)
                    out.append(("resblock", precision, res[m], c, 1, out_act, x_act))
                else:
                    conv(c, c, k, d)
                    conv(c, c, k, 1)
    conv(1, ch[-1], 7, 1, post=True)
    return out


def plan(cfg, precision, knob, limit):
    """the launch record fs2_voc_last_launches should hold after a synthesize of `cfg` under (knob, limit)"""
    with knobs(knob, limit) as lib:
        out = []
        for l in layers(lib, cfg, precision, knob):
            if l[0] == "conv":
                _, n, cin, taps, dil, shift, post, in_fp32 = l
                l = ("conv", precision) + conv_tile(lib, precision, n, cin, taps, dil, shift, post) + (in_fp32, post, shift)
            out.append(l)
        return out


def instantiation(launch):
    return launch[:4] if launch[0] == "conv" else launch[:6]


def compiled():
    """every instantiation the launchers can name (launch_vocoder_conv: 3 types x 4 heights x 6 strides; launch_vocoder_resblock:
    3 types x 3 forms x 3 widths, a block, a raw-storing pair or an activated-storing pair)"""
    s = {("conv", dt, mi, cp) for dt in DTYPES for mi in (14, 8, 4, 2) for cp in (0,) + CP_BUILDS}
    s |= {("resblock", dt, f, c, n, mid) for dt in DTYPES for f in (408, 808, 804) for c in (32, 64, 128)
          for n, mid in ((3, False), (1, False), (1, True))}
    return s


# ---- the two pinned tables: tests/test_voc_forms_cpu.py holds the pickers to them, tests/test_gpu_hifigan_forms.py runs the first -----
_ALL_CP = (0, 32, 64, 128, 256, 512)
_PAIRS_AND_BLOCKS = tuple((c, n, mid) for c in (32, 64, 128) for n, mid in ((1, False), (1, True), (3, False)))


def _table(conv, rb):
    """{(precisions, MI16): CPs}, {(precisions, form): [(channels, npairs, MID)]} -> a set of instantiations"""
    s = {("conv", dt, mi, cp) for (dts, mi), cps in conv.items() for dt in dts for cp in cps}
    return s | {("resblock", dt, f, c, n, mid) for (dts, f), shapes in rb.items() for dt in dts for c, n, mid in shapes}


_16, _32 = ("bf16", "fp16"), ("fp32",)
# Reached by a config of CONFIGS under some (resblock knob, LDS limit 0..150).  bf16 and fp16 share tiles, LDS sizes and grids.
REACHABLE = _table(
    {(_16, 2): _ALL_CP, (_16, 4): _ALL_CP, (_16, 8): (32, 64, 128, 256, 512), (_16, 14): (32, 64, 128, 256),
     (_32, 2): _ALL_CP, (_32, 4): (32, 64, 128, 256, 512), (_32, 8): (32, 64, 128, 256), (_32, 14): (128,)},
    {(_16, 408): [s for s in _PAIRS_AND_BLOCKS if s != (128, 3, False)],   # a whole 128-channel block: see UNREACHABLE
     (_16, 808): _PAIRS_AND_BLOCKS,
     (_16, 804): [(128, 1, False)],                                        # the k = 11, dilation 9 pair: 808's slabs would take 153 KiB
     (_32, 804): _PAIRS_AND_BLOCKS})
# Compiled (launch_vocoder_conv / launch_vocoder_resblock can name them), reached by none of these geometries:
#  - the runtime-stride build above the height a 1024-channel slab leaves room for (150 KiB: 64 rows of 2-byte, 32 of 4-byte elements);
#  - the tallest conv tiles at the widest strides: 16 * 14 * WM rows x CP no longer fit 150 KiB;
#  - fp32 resident tiles other than 804: the 4-wave form's two slabs exceed 76 KiB, the full-height 8-wave form's 150 KiB, at every width;
#  - a whole 128-channel block on 4 waves: only knob 7 launches one, and at k = 3 its halo leaves 83 % of the 128 rows, under the 85 % that
#    only the percentage knob lowers;
#  - 16-bit 804 wherever 808 fits (it is tried first), i.e. everywhere but the one long-dilation pair; that pair (the
#    longest dilation) is the last of its block, so it never stores activated.
UNREACHABLE = _table(
    {(_16, 8): (0,), (_16, 14): (0, 512), (_32, 4): (0,), (_32, 8): (0, 512), (_32, 14): (0, 32, 64, 256, 512)},
    {(_16, 408): [(128, 3, False)],
     (_16, 804): [s for s in _PAIRS_AND_BLOCKS if s != (128, 1, False)],
     (_32, 408): _PAIRS_AND_BLOCKS, (_32, 808): _PAIRS_AND_BLOCKS})


def inputs(name):
    """(cfg, weights, mel, lengths) of a config of CONFIGS"""
    from lightningfastspeech2_amd.hifigan import synth_state_dict
    cfg, seed, mel_seed, T, lengths = CONFIGS[name]
    return cfg, synth_state_dict(cfg, seed), _voc16.random_mel(mel_seed, len(lengths), T), torch.tensor(lengths, dtype=torch.int32)
