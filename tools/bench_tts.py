#!/usr/bin/env python
"""End-to-end text-to-waveform throughput on one MI355X: FastSpeech2 mel forward (bench.py's workload: FS2-27M,
batch 32 x 256 phonemes, 6 frames/phoneme -> 1536 frames each) followed by the HiFi-GAN V1 generator on the
padded mel batch with its valid frame counts (SpeechGenerator.generate_samples without the host loop); bf16 by default,
--precision mixed16 / --vocoder-precision fp16 for the binary16-storage decoder and generator.
Prints ONE JSON line.  Random-init weights, synthetic inputs, everything resident in HBM.

--to-host names where a step ends (a comma-separated list, or "all"): "off" (default) at the device waveform, as above; "device" at the
per-utterance float32 numpy arrays of SpeechGenerator.generate_samples (cast, rescale and packing on the device, one pinned copy);
"pipeline" the same through SpeechGenerator.pipeline(2) (views of its pinned ring); "legacy" the host recipe generate_samples used
before - padded fp32 .cpu(), numpy cast over the pads, slice, astype / 32767 - kept here only as the yardstick.  With anything but
plain "off" the modes alternate inside each of --loops (5) loops of --steps steps in this one process; one JSON line per mode with
every loop's time and the fastest as the figure, then one line with fs2_op_wav_pack's own launch time on the step's waveform."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from lightningfastspeech2_amd.config import preset
from lightningfastspeech2_amd.hifigan import HifiGan, HifiGanConfig, synth_state_dict as voc_sd, wav_pack
from lightningfastspeech2_amd.model import FastSpeech2
from lightningfastspeech2_amd.synthesis import SpeechGenerator
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phones", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "mixed16"], help="the mel forward's mode")
    ap.add_argument("--vocoder-precision", default="bf16", choices=["bf16", "fp16"], help="the generator's storage type")
    ap.add_argument("--to-host", default="off", help="off | legacy | device | pipeline, comma-separated, or all")
    ap.add_argument("--loops", type=int, default=5, help="loops per mode when --to-host is more than plain off")
    a = ap.parse_args()
    modes = ["off", "legacy", "device", "pipeline"] if a.to_host == "all" else a.to_host.split(",")
    if any(m not in ("off", "legacy", "device", "pipeline") for m in modes):
        ap.error(f"--to-host {a.to_host!r}")
    cfg = preset("c2")
    model = FastSpeech2(cfg, synth_state_dict(cfg, 0, duration_bias=math.log(7.0), duration_weight_scale=0.0), precision=a.precision)
    vcfg = HifiGanConfig()
    voc = HifiGan(vcfg, voc_sd(vcfg, 0), precision=a.vocoder_precision)
    inp = synth_inputs(cfg, a.batch, a.phones, seed=1234)
    batch = {"phones": torch.from_numpy(inp["phones"]).cuda(), "speaker": torch.from_numpy(inp["speaker"]).cuda()}

    def step():
        out = model(batch, inference=True)
        lengths = (~out["tgt_mask"]).sum(dim=1).to(torch.int32)
        return out, voc.synthesize(out["mel"], lengths)

    if modes != ["off"]:
        return to_host(a, modes, model, voc, vcfg, batch, step)
    for _ in range(a.warmup):
        out, wav = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out, wav = step()
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / a.steps
    frames = int((~out["tgt_mask"]).sum())
    samples = frames * vcfg.hop
    print(json.dumps({"metric": "audio samples/sec, phonemes -> waveform (FastSpeech2 FS2-27M + HiFi-GAN V1)", "value": samples / el,
                      "unit": "samples/s", "ms_per_step": el * 1e3, "audio_seconds_per_step": samples / vcfg.sampling_rate,
                      "rtf": el / (samples / vcfg.sampling_rate), "mel_frames_per_s": frames / el, "n_gpus": 1,
                      "dtype": a.precision if a.precision == a.vocoder_precision else f"{a.precision}+{a.vocoder_precision}",
                      "data": "synthetic", "steps": a.steps, "warmup": a.warmup,
                      "config": {"workload": f"batch {a.batch} x {a.phones} phonemes -> {frames // a.batch} frames -> "
                                             f"{samples // a.batch} samples per utterance, random-init weights"}}), flush=True)


def to_host(a, modes, model, voc, vcfg, batch, step):
    gen = SpeechGenerator(model, voc)
    pipe = gen.pipeline(2) if "pipeline" in modes else None
    hop = vcfg.hop

    def legacy():
        out, wav = step()
        lengths = (~out["tgt_mask"]).sum(dim=1).to(torch.int32)
        i16 = (wav.cpu().numpy() * 32768.0).astype("int16")
        return [i16[b, :int(n) * hop].astype(np.float32) / 32767.0 for b, n in enumerate(lengths.tolist())]

    def loop(mode, steps):
        """-> seconds per step, samples handed over per step"""
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "pipeline":
            for _ in range(steps):
                for res in pipe.submit(batch):
                    n += sum(len(x) for x in res["audios"])
            for res in pipe.drain():
                n += sum(len(x) for x in res["audios"])
        else:
            for _ in range(steps):
                if mode == "off":
                    out, _ = step()
                elif mode == "legacy":
                    n += sum(len(x) for x in legacy())
                else:
                    n += sum(len(x) for x in gen.generate_samples(batch)["audios"])
            torch.cuda.synchronize()
            if mode == "off":
                n = int((~out["tgt_mask"]).sum()) * hop * steps
        return (time.perf_counter() - t0) / steps, n // steps

    for m in modes:
        loop(m, a.warmup)
    times, samples = {m: [] for m in modes}, {}
    for _ in range(a.loops):
        for m in modes:  # alternating: every mode sees the same clocks and the same neighbours
            el, samples[m] = loop(m, a.steps)
            times[m].append(el)
    dt = a.precision if a.precision == a.vocoder_precision else f"{a.precision}+{a.vocoder_precision}"
    for m in modes:
        el = min(times[m])
        print(json.dumps({"metric": "audio samples/sec, phonemes -> waveform (FastSpeech2 FS2-27M + HiFi-GAN V1)", "to_host": m,
                          "value": samples[m] / el, "unit": "samples/s", "ms_per_step": el * 1e3,
                          "loops_ms_per_step": [round(t * 1e3, 3) for t in times[m]],
                          "audio_seconds_per_step": samples[m] / vcfg.sampling_rate, "rtf": el / (samples[m] / vcfg.sampling_rate),
                          "n_gpus": 1, "dtype": dt, "data": "synthetic", "steps": a.steps, "warmup": a.warmup, "loops": a.loops,
                          "config": {"workload": f"batch {a.batch} x {a.phones} phonemes -> {samples[m] // a.batch} samples per "
                                                 f"utterance, random-init weights"}}), flush=True)
    if pipe is not None:
        pipe.close()
    # the pack launch alone, on the step's own waveform and frame counts (device events around 20 launches, fastest of five)
    out, wav = step()
    lengths = (~out["tgt_mask"]).sum(dim=1).to(torch.int32)
    pack_us = {}
    for kind in ("int16", "float32"):
        buf = torch.empty(wav.numel(), dtype=torch.int16 if kind == "int16" else torch.float32, device=wav.device)
        best = float("inf")
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                wav_pack(wav, lengths, hop, kind, out=buf)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / 20 * 1e3)
        pack_us[kind] = round(best, 2)
    mb = {k: int(lengths.sum()) * hop * (4 + (2 if k == "int16" else 4)) / 1e6 for k in pack_us}  # pads are neither read nor written
    print(json.dumps({"metric": "fs2_op_wav_pack launch, us (20 back-to-back launches between device events, fastest of 6)",
                      "value": pack_us, "unit": "us", "megabytes_moved": mb,
                      "shape": [int(wav.shape[0]), int(wav.shape[1])], "hop": hop}), flush=True)


if __name__ == "__main__":
    main()
