#!/usr/bin/env python3
"""The precision modes side by side on one GPU: time and distance to the oracle's mel, from one process on one box.

    python tools/bench_precision.py [--config c2|ref-default|c3] [--batch 32] [--steps 20] [--repeats 5] [--warmup 3] [--sample 4]

Per mode in bf16, mixed3, mixed16, fp32x3 one JSON line:
  ms_per_batch_one_in_flight / ms_per_batch_two_in_flight   bench.py's workload (B utterances x 256 phones x 6 frames per phone),
                                                            timed as bench.py's parity block times a mode: synchronous forwards,
                                                            then model.pipeline(2); the fastest of --repeats loops each (all listed)
  mel_max_forced / mel_mean_forced                          |mel - oracle| under the oracle's durations and buckets, on the first
                                                            --sample utterances of the batch (the CPU oracle finishes them in well
                                                            under a minute)
  duration_flips / bucket_flips                             free-running decisions against the oracle's on the same sample
Boxes differ by ~8 %: only figures of one run compare.  No CPU-baseline sweep, no profiler run; bench.py stays the headline.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ["bf16", "mixed3", "mixed16", "fp32x3"]


def timed(model, full, n, warmup, repeats):
    """ms per batch of `repeats` loops of n forwards, one at a time and two in flight (all repeats; the caller reports the fastest)"""
    for _ in range(warmup):
        model(full, inference=True)
    one, piped = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            model(full, inference=True)
        torch.cuda.synchronize()
        one.append((time.perf_counter() - t0) / n * 1e3)
    pipe = model.pipeline(2)
    try:
        for _ in range(4):
            pipe.submit(full)
        pipe.drain()
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2 * n):
                pipe.submit(full)
            pipe.drain()
            torch.cuda.synchronize()
            piped.append((time.perf_counter() - t0) / (2 * n) * 1e3)
    finally:
        pipe.close()
    return one, piped


def build_stamp():
    """What the library was built from (lightningfastspeech2_amd/_build_info.json, written by build()) and whether that still
    describes the kernel sources next to it: a stale stamp is reported as such, never passed on as the measured commit."""
    import hashlib
    csrc = os.path.join(ROOT, "lightningfastspeech2_amd", "csrc")
    now = {f: hashlib.sha256(open(os.path.join(csrc, f), "rb").read()).hexdigest()[:16] for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    digest = hashlib.sha256("".join(f + now[f] for f in now).encode()).hexdigest()[:16]
    try:
        with open(os.path.join(ROOT, "lightningfastspeech2_amd", "_build_info.json")) as f:
            bi = json.load(f)
    except OSError:
        return {"head": None, "kernel_sources_sha256": digest, "stamp": "missing"}
    stale = bi.get("kernel_sha256") != now
    return {"head": bi.get("head"), "dirty": bi.get("dirty"), "kernel_sources_sha256": digest,
            "stamp": "STALE: the kernel sources differ from the ones the stamp was written for" if stale else "matches the kernel sources"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "ref-default", "c3"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phones", type=int, default=256)
    ap.add_argument("--frames-per-phone", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5, help="timed loops per figure; the fastest is reported, all are listed")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=4, help="utterances of the batch compared with the CPU oracle")
    ap.add_argument("--modes", default=",".join(MODES))
    args = ap.parse_args()

    from lightningfastspeech2_amd.config import preset
    from lightningfastspeech2_amd.model import FastSpeech2
    from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
    from oracle import oracle_cpu  # checker only

    dev = torch.device("cuda:0")
    cfg = preset(args.config)
    sd = synth_state_dict(cfg, 0, duration_bias=math.log(1.0 + args.frames_per_phone), duration_weight_scale=0.0)  # bench.py's workload
    inp = synth_inputs(cfg, args.batch, args.phones, seed=1234)
    full = {"phones": torch.from_numpy(inp["phones"]).to(dev), "speaker": torch.from_numpy(inp["speaker"]).to(dev)}
    Bs = max(1, min(args.sample, args.batch))
    ph, sp = inp["phones"][:Bs], inp["speaker"][:Bs]
    t0 = time.perf_counter()
    ref = oracle_cpu.forward(sd, cfg, ph, sp, return_intermediates=True)
    oracle_s = time.perf_counter() - t0
    ref_b = {v: ref["_intermediates"][f"bucket_{v}"] for v in cfg.variances}
    sample = {"phones": torch.from_numpy(ph).to(dev), "speaker": torch.from_numpy(sp).to(dev)}
    build = build_stamp()
    print(json.dumps({"tool": "bench_precision", "config": args.config, "batch": args.batch, "phones": args.phones,
                      "frames": int(ref["mel"].shape[1]), "sample_utterances": Bs, "oracle_seconds": round(oracle_s, 2),
                      "mel_scale": float(ref["mel"].abs().max()), "device": torch.cuda.get_device_name(0), "build": build}), flush=True)
    for mode in [m for m in args.modes.split(",") if m]:
        model = FastSpeech2(cfg, sd, precision=mode, device=dev)
        model.engine.set_debug(True)
        out = model(sample, inference=True)
        dfl = int((out["duration_rounded"].cpu() != ref["duration_rounded"]).sum())
        bfl = -1
        if dfl == 0 and out["mel"].shape == ref["mel"].shape:
            bfl = sum(int((model.engine.debug_tensor(f"bucket_{v}").cpu().long() != ref_b[v]).sum()) for v in cfg.variances)
        model.engine.set_debug(False)
        e = (model.forward(sample, force_durations=ref["duration_rounded"], force_buckets=ref_b)["mel"].cpu() - ref["mel"]).abs()
        one, piped = timed(model, full, args.steps, args.warmup, args.repeats)
        print(json.dumps({"mode": mode, "ms_per_batch_one_in_flight": round(min(one), 4), "ms_per_batch_two_in_flight": round(min(piped), 4),
                          "repeats_one_in_flight": [round(t, 4) for t in one], "repeats_two_in_flight": [round(t, 4) for t in piped],
                          "mel_max_forced": float(e.max()), "mel_mean_forced": float(e.mean()), "duration_flips": dfl, "bucket_flips": bfl,
                          "buckets_compared": int(sum(ref_b[v].numel() for v in cfg.variances))}), flush=True)
        del model
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
