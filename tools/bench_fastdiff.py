#!/usr/bin/env python
"""FastDiff inference on an MI355X: ms per batch (default 32 x 1536 frames, N = 4) in bf16 and fp32, beside the HiFi-GAN V1 pass
of the same process; fastest of --loops loops each.  The share of the kernel predictors and of the LVC launches is measured by
running those launches alone on the same shapes (fs2_fd_predict_kernels, fs2_op_lvc), chunk by chunk as the engine walks the
batch; "rest" is the remainder.  FLOPs are the algorithmic count of the architecture (2 x multiply-adds, transposed convolutions
at their two live taps).  Prints one JSON line per precision.

    python tools/bench_fastdiff.py [--batch 32] [--frames 1536] [--steps 4] [--loops 5] [--precisions bf16 fp32]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lightningfastspeech2_amd import fastdiff as FD  # noqa: E402
from lightningfastspeech2_amd.hifigan import HifiGan, HifiGanConfig, synth_state_dict as voc_sd  # noqa: E402


def flops_per_frame():
    """algorithmic FLOPs of one eps evaluation per mel frame, by launch class"""
    kp = 3 * 2 * (80 * 64 * 5 + 6 * 64 * 64 * 3 + 64 * 24576 * 3 + 64 * 256 * 3)
    rows = 8 + 64 + 256
    lvc = rows * 4 * 2 * 96 * 64
    dil = rows * 4 * 2 * 32 * 32 * 3
    rest = rows * 2 * 32 * 32 * 2 + (64 + 8 + 1) * 2 * (3 * 32 * 32 * 3 + 32 * 32) + 256 * 2 * 2 * 7 * 32
    return {"kernel_predictor": kp, "lvc": lvc, "dilated_convs": dil, "other": rest}


def fastest(fn, loops):
    best = float("inf")
    for _ in range(loops):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1536)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--precisions", nargs="+", default=["bf16", "fp32"])
    a = ap.parse_args()
    B, T, N = a.batch, a.frames, a.steps
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    mel = torch.randn(B, T, 80, generator=g).to(dev)
    noise = torch.randn(N, B, T * 256, generator=g).to(dev)
    cfg = FD.FastDiffConfig()
    sd = FD.synth_state_dict(cfg, 0)
    fl = flops_per_frame()
    total_flop = sum(fl.values()) * B * T * N
    voc = HifiGan(HifiGanConfig(), voc_sd(HifiGanConfig(), 0), precision="bf16", device=dev)
    voc.synthesize(mel)
    hifigan_ms = fastest(lambda: voc.synthesize(mel), a.loops)
    for prec in a.precisions:
        fd = FD.FastDiff(cfg, sd, precision=prec, device=dev)
        wav = torch.empty(B, T * 256, device=dev)
        fd.inference(mel, None, N=N, noise=noise, out=wav)  # warm-up: workspace, code objects
        total = fastest(lambda: fd.inference(mel, None, N=N, noise=noise, out=wav), a.loops)
        # the kernel predictors alone: three blocks per step
        td = torch.bfloat16 if prec == "bf16" else torch.float32
        Kf, kbf = torch.empty(B, T, 24576, device=dev, dtype=td), torch.empty(B, T, 256, device=dev, dtype=td)
        ws, stream = fd._workspace(fd.workspace_bytes(B, T)), torch.cuda.current_stream()

        def predict():
            for blk in range(3):
                fd._check(fd.lib.fs2_fd_predict_kernels(fd.handle, blk, mel, None, 74.99, Kf, kbf, ws, ws.numel(), B, T, stream), "predict")
        kp = fastest(predict, a.loops) * N
        del Kf, kbf
        # the LVC launches alone, on one chunk's shapes, scaled to the batch
        es = 2 if prec == "bf16" else 4
        Bc = max(1, min(B, fd.workspace_bytes(B, T) // fd.workspace_bytes(1, T)))
        K = torch.randn(Bc, T, 24576, device=dev).to(td) * 0.1
        kb = torch.zeros(Bc, T, 256, device=dev, dtype=td)
        lvc_ms = 0.0
        for hop in (8, 64, 256):
            y = torch.randn(Bc, T * hop, 32, device=dev).to(td)
            x = torch.zeros_like(y)
            FD.lvc(y, K, kb, x, None, None, hop, 0, prec)
            lvc_ms += fastest(lambda: [FD.lvc(y, K, kb, x, None, None, hop, i, prec) for i in range(4)], a.loops)
            del y, x
        lvc_ms *= N * B / Bc
        kbytes = 3 * N * B * T * 24576 * es * 2  # the predicted-kernel tensor: written once by kernel_conv, read once by the LVC
        print(json.dumps({
            "bench": "fastdiff_inference", "precision": prec, "batch": B, "frames": T, "steps": N, "loops": a.loops,
            "ms_per_batch": round(total, 2), "kernel_predictor_ms": round(kp, 2), "lvc_ms": round(lvc_ms, 2),
            "rest_ms": round(total - kp - lvc_ms, 2), "chunk_utterances": int(Bc), "launches_per_chunk": fd.launches(N),
            "algorithmic_tflop": round(total_flop / 1e12, 3), "tflops_achieved": round(total_flop / total / 1e9, 2),
            "kernel_predictor_tflops": round(fl["kernel_predictor"] * B * T * N / kp / 1e9, 2),
            "lvc_tflops": round(fl["lvc"] * B * T * N / lvc_ms / 1e9, 2),
            "predicted_kernel_traffic_gb": round(kbytes / 1e9, 2), "predicted_kernel_gbps_over_total": round(kbytes / total / 1e6, 1),
            "hifigan_v1_bf16_ms": round(hifigan_ms, 2), "audio_seconds": round(B * T * 256 / 22050, 1)}), flush=True)
        del fd, K, kb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
