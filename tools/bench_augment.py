#!/usr/bin/env python
"""Augmentation on the device (lightningfastspeech2_amd/augment.py, csrc/augment.hip) at the speech pipeline's batch: 32 utterances x
393,216 samples (bench_tts.py's workload).  One JSON line per figure:

- each operation alone on a packed float32 buffer of that size (device events around --reps back-to-back calls, fastest of --loops):
  resample 22050 -> 16000, impulse responses of 4096 and 16384 taps (with the achieved fraction of the 155 TFLOP/s the project
  measured for v_mfma_f32_32x32x2_f32, profiles/analysis_front_end.md, counting 2 R flops per output), noise;
- SpeechGenerator.pipeline(2) per batch without and with Resample + RoomImpulse(4096 taps, p = 1) + GaussianSNR(p = 1), both
  alternating inside each of --loops loops in this one process, fastest loop each: only figures of one run compare;
- the host recipe on the same box for the same 32 arrays, 16 threads at most: scipy.signal.fftconvolve (numpy's FFT where scipy
  is absent), a numpy polyphase loop over the same table, numpy noise.
Random-init weights, synthetic responses (augment.synthetic_rir: a test signal, not a room model)."""
import argparse
import concurrent.futures as cf
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from lightningfastspeech2_amd.augment import (DeviceAugment, GaussianSNR, Resample, RoomImpulse, resample_params, resample_table,
                                              synthetic_rir, wav_add_noise, wav_convolve, wav_resample)

MFMA_FP32_TFLOPS = 155.0  # profiles/analysis_front_end.md


def emit(**kw):
    print(json.dumps(kw), flush=True)


def device_time(fn, reps, loops):
    """ms per call: device events around `reps` back-to-back calls, fastest of `loops`"""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(loops):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def ops_alone(a):
    B, n = a.batch, a.samples
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    packed = 0.1 * torch.randn(B * n, generator=g, device=dev)
    offsets = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    shape = {"batch": B, "samples": n}
    orig, new, width, K = resample_params(22050, 16000)
    tab = torch.from_numpy(resample_table(22050, 16000).astype(np.float32)).to(dev)
    out = torch.empty(B * (-(-new * n // orig)), dtype=torch.float32, device=dev)
    ms = device_time(lambda: wav_resample(packed, offsets, n, tab, orig, new, width, out=out), a.reps, a.loops)
    emit(metric="fs2_op_wav_resample 22050 -> 16000, ms", value=round(ms, 4), unit="ms", taps=K,
         mfma_fraction=round(2.0 * out.numel() * K / (ms * 1e-3) / (MFMA_FP32_TFLOPS * 1e12), 4), **shape)
    out = torch.empty(B * n, dtype=torch.float32, device=dev)
    for R in (4096, 16384):
        bank = torch.from_numpy(synthetic_rir(R, 6.0 / R, 1)[None]).to(dev)
        lens = torch.tensor([R], dtype=torch.int32, device=dev)
        idx = torch.zeros(B, dtype=torch.int32, device=dev)
        ms = device_time(lambda: wav_convolve(packed, offsets, n, bank, lens, idx, "same", out=out), a.reps, a.loops)
        tflops = 2.0 * B * n * R / (ms * 1e-3) / 1e12
        emit(metric=f"fs2_op_wav_convolve, {R} taps, same, ms", value=round(ms, 4), unit="ms", tflops=round(tflops, 2),
             mfma_fraction=round(tflops / MFMA_FP32_TFLOPS, 4), **shape)
    z = torch.randn(B * n, generator=g, device=dev)
    snr = torch.full((B,), 15.0, dtype=torch.float32, device=dev)
    ms = device_time(lambda: wav_add_noise(packed, offsets, n, z, snr, out=out), a.reps, a.loops)
    emit(metric="fs2_op_wav_add_noise, ms", value=round(ms, 4), unit="ms", gbytes_per_s=round(B * n * 16 / (ms * 1e-3) / 1e9, 1), **shape)


def host_recipe(a):
    try:
        from scipy.signal import fftconvolve
        conv_name = "scipy.signal.fftconvolve"
    except ImportError:
        conv_name = "numpy rfft (scipy is absent)"

        def fftconvolve(x, h):
            nfft = 1 << (len(x) + len(h) - 2).bit_length()
            return np.fft.irfft(np.fft.rfft(x, nfft) * np.fft.rfft(h, nfft), nfft)[:len(x) + len(h) - 1]
    B, n = a.batch, a.samples
    rng = np.random.default_rng(0)
    xs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(B)]
    h = synthetic_rir(4096, 6.0 / 4096, 1)
    orig, new, width, K = resample_params(22050, 16000)
    tab = resample_table(22050, 16000).astype(np.float32)

    def polyphase(x):
        frames = -(-(-(-new * len(x) // orig)) // new)
        xp = np.zeros(width + frames * orig + K, np.float32)
        xp[width:width + len(x)] = x
        F = np.lib.stride_tricks.as_strided(xp, (frames, K), (orig * 4, 4))
        y = np.empty((frames, new), np.float32)
        for p in range(new):
            y[:, p] = F @ tab[p]
        return y.reshape(-1)[:-(-new * len(x) // orig)]

    def noise(x, seed):
        z = np.random.default_rng(seed).standard_normal(len(x)).astype(np.float32)
        return x + np.float32(np.sqrt(np.mean(x.astype(np.float64) ** 2)) / 10.0 ** (15.0 / 20.0)) * z

    def whole(i):
        return noise(fftconvolve(polyphase(xs[i]), h)[:-(-new * n // orig)].astype(np.float32), i)

    try:  # 16 pool threads, one BLAS thread each where that can be arranged: 16 threads at most
        from threadpoolctl import threadpool_limits
        threadpool_limits(1)
    except ImportError:
        pass
    with cf.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for name, fn in (("numpy polyphase resample 22050 -> 16000", lambda i: polyphase(xs[i])),
                         (f"{conv_name}, 4096 taps", lambda i: fftconvolve(xs[i], h)[:n]),
                         ("numpy Gaussian noise at an SNR", lambda i: noise(xs[i], i)),
                         ("host recipe: resample + response + noise", whole)):
            best = float("inf")
            for _ in range(max(a.loops // 2, 2)):
                t0 = time.perf_counter()
                list(pool.map(fn, range(B)))
                best = min(best, time.perf_counter() - t0)
            emit(metric=f"host, {name}, ms per batch (16 threads at most)", value=round(best * 1e3, 2), unit="ms", batch=B, samples=n)


def pipeline(a):
    from lightningfastspeech2_amd.config import preset
    from lightningfastspeech2_amd.hifigan import HifiGan, HifiGanConfig, synth_state_dict as voc_sd
    from lightningfastspeech2_amd.model import FastSpeech2
    from lightningfastspeech2_amd.synthesis import SpeechGenerator
    from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
    cfg = preset("c2")
    model = FastSpeech2(cfg, synth_state_dict(cfg, 0, duration_bias=math.log(7.0), duration_weight_scale=0.0), precision="bf16")
    vcfg = HifiGanConfig()
    voc = HifiGan(vcfg, voc_sd(vcfg, 0), precision="bf16")
    inp = synth_inputs(cfg, a.batch, 256, seed=1234)
    batch = {"phones": torch.from_numpy(inp["phones"]).cuda(), "speaker": torch.from_numpy(inp["speaker"]).cuda()}
    aug = DeviceAugment([Resample(22050, 16000), RoomImpulse([synthetic_rir(4096, 6.0 / 4096, s) for s in range(4)], p=1.0),
                         GaussianSNR(5.0, 30.0, p=1.0)], seed=0)
    pipes = {"plain": SpeechGenerator(model, voc).pipeline(2), "augmented": SpeechGenerator(model, voc, augmentations=aug).pipeline(2)}

    def loop(pipe, steps):
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            for res in pipe.submit(batch):
                n += sum(len(x) for x in res["audios"])
        for res in pipe.drain():
            n += sum(len(x) for x in res["audios"])
        return (time.perf_counter() - t0) / steps, n // steps

    for p in pipes.values():
        loop(p, a.warmup)
    times, samples = {m: [] for m in pipes}, {}
    for _ in range(a.loops):
        for m, p in pipes.items():  # alternating: both modes see the same clocks and the same neighbours
            el, samples[m] = loop(p, a.steps)
            times[m].append(el)
    for p in pipes.values():
        p.close()
    for m in pipes:
        emit(metric=f"SpeechGenerator.pipeline(2), {m}, ms per batch", value=round(min(times[m]) * 1e3, 3), unit="ms",
             loops_ms_per_batch=[round(t * 1e3, 3) for t in times[m]], samples_per_batch=samples[m], steps=a.steps, loops=a.loops)
    emit(metric="augmentation in the pipeline, ms per batch over plain (same run)",
         value=round((min(times["augmented"]) - min(times["plain"])) * 1e3, 3), unit="ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=393216)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="ops,pipeline,host", help="comma-separated: ops, pipeline, host")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if "ops" in parts:
        ops_alone(a)
    if "pipeline" in parts:
        pipeline(a)
    if "host" in parts:
        host_recipe(a)


if __name__ == "__main__":
    main()
