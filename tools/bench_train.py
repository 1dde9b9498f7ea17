#!/usr/bin/env python
"""Training-step timing on synthetic data: teacher-forced forward + losses + backward + optimizer step.
    python tools/bench_train.py [--config c2] [--batch 32] [--phones 256] [--steps 5] [--warmup 2]
Prints one JSON line: ms per step, mel frames per second through the training step, and the split forward / backward.
    --class-default-variances   the chosen config with the reference's class-default variance set (pitch phone + cwt, energy phone,
                                snr phone) timed IN THE SAME PROCESS as the config's own frame-level step, the fastest of five
                                loops of --steps each (tools/bench_precision.py's convention; boxes differ by ~8 %), plus the
                                per-launch times of fs2_op_cwt_head_train / fs2_op_cwt_head_bwd at the phone-level (B L rows)
                                and frame-level (B T rows) shapes: a second JSON line."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightningfastspeech2_amd.config import preset  # noqa: E402
from lightningfastspeech2_amd.training import Trainer  # noqa: E402
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phones", type=int, default=256)
    ap.add_argument("--frames-per-phone", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--dropout", type=float, default=0.0, help="every nn.Dropout site of the reference at this rate (the shipped recipe: 0.1)")
    ap.add_argument("--class-default-variances", action="store_true")
    ap.add_argument("--knob", type=int, action="append", default=[], help="fs2_op_set_gemm_variant values (A/B switches)")
    a = ap.parse_args()
    for k in a.knob:
        from lightningfastspeech2_amd import _lib
        _lib.load().fs2_op_set_gemm_variant(k)
    cfg = preset(a.config)
    B, L = a.batch, a.phones
    T = L * a.frames_per_phone
    inp = synth_inputs(cfg, B, L, seed=1234)
    rs = np.random.RandomState(5)
    batch = {"phones": torch.from_numpy(inp["phones"]).cuda(), "speaker": torch.from_numpy(inp["speaker"]).cuda(),
             "duration": torch.full((B, L), a.frames_per_phone, dtype=torch.int64).cuda(),
             "mel": torch.from_numpy((rs.randn(B, T, cfg.n_mels) - 2).astype(np.float32)).cuda()}
    for v in cfg.variances:
        batch[f"variances_{v}"] = torch.from_numpy(rs.randn(B, T).astype(np.float32)).cuda()
    kw = {} if a.precision == "fp32" else {"precision": a.precision}
    if a.dropout > 0:
        kw.update(encoder_dropout=a.dropout, decoder_dropout=a.dropout, variance_dropout=a.dropout, duration_dropout=a.dropout)
    if a.class_default_variances:
        return class_default(a, cfg, batch, kw, B, L, T, rs)
    sd = synth_state_dict(cfg, 0, duration_bias=math.log(7.0), duration_weight_scale=0.0)
    tr = Trainer(cfg, sd, **kw)
    for _ in range(a.warmup):
        losses = tr.training_step(batch)
        tr.optimizer_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        losses = tr.training_step(batch)
        tr.optimizer_step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    print(json.dumps({"metric": "training step (forward + loss + backward + AdamW)", "config": a.config, "batch": B, "phones": L,
                      "frames": T, "precision": a.precision, "ms_per_step": dt * 1e3, "mel_frames_per_s": B * T / dt,
                      "loss_total": float(losses["total"]), "peak_mem_GB": torch.cuda.max_memory_allocated() / 2**30}))


def loops(tr, batch, steps, warmup, repeats=5):
    for _ in range(warmup):
        tr.training_step(batch)
        tr.optimizer_step()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.training_step(batch)
            tr.optimizer_step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def op_times(precision, B, S, F, n=20):
    """us per launch of the two CWT-head operators on (B S, F) rows (events around n launches, the fastest of five)"""
    from lightningfastspeech2_amd import _lib
    lib = _lib.load()
    dt, tdt = (_lib.FS2_F32, torch.float32) if precision == "fp32" else (_lib.FS2_BF16, torch.bfloat16)
    z = lambda *s, dtype=torch.float32: torch.randn(*s, device="cuda").to(dtype)
    y, w10, b10, msw, msb = z(B * S, F, dtype=tdt), z(10, F), z(10), z(2, F), z(2)
    mask = torch.zeros(B * S, dtype=torch.uint8, device="cuda")
    spec, ybar, ms, dy = z(B * S, 10), z(B, F), z(B, 2), z(B * S, F, dtype=tdt)
    g = [z(10, F), z(10), z(2, F), z(2)]
    ws1 = torch.zeros(int(lib.fs2_op_cwt_head_train_ws_bytes(B, S, F)) // 4 + 1, device="cuda")
    ws2 = torch.zeros(int(lib.fs2_op_cwt_head_bwd_ws_bytes(B, S, F)) // 4 + 1, device="cuda")
    st = torch.cuda.current_stream()
    fwd = lambda: _lib.check(lib.fs2_op_cwt_head_train(dt, y, w10, b10, msw, msb, mask, spec, ybar, ms, ws1, B, S, F, st))
    bwd = lambda: _lib.check(lib.fs2_op_cwt_head_bwd(dt, y, spec, ms, ybar, w10, msw, dy, g[0], g[1], g[2], g[3], ws2, B, S, F, st))
    out = {}
    for name, fn in (("cwt_head_train_us", fwd), ("cwt_head_bwd_us", bwd)):
        fn()
        best = None
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) / n * 1e3
            best = t if best is None else min(best, t)
        out[name] = best
    out["tensor_MB"] = B * S * F * y.element_size() / 1e6
    return out


def class_default(a, cfg, batch, kw, B, L, T, rs):
    import dataclasses
    nv = len(cfg.variances)
    stats = dict(cfg.stats)
    stats[cfg.variances[0]] = dict(stats[cfg.variances[0]], min=0.2, max=5.0)  # a CWT variance is bucketised in the log domain
    cd = dataclasses.replace(cfg, variance_levels=["phone"] * nv, variance_transforms=["cwt"] + ["none"] * (nv - 1), stats=stats)
    v0 = cfg.variances[0]
    cdb = {k: v for k, v in batch.items() if not k.startswith("variances_")}
    f = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).cuda()
    cdb.update({f"variances_{v0}_signal": torch.exp(0.5 * f(B, L)), f"variances_{v0}_spectrogram": f(B, L, 10),
                f"variances_{v0}_mean": f(B), f"variances_{v0}_std": f(B).abs() + 0.5})
    for v in cfg.variances[1:]:
        cdb[f"variances_{v}"] = f(B, L)
    res = {"metric": "training step, class-default variances vs the config's frame-level step (same process, fastest of 5 loops)",
           "config": a.config, "batch": B, "phones": L, "frames": T, "precision": a.precision, "dropout": a.dropout}
    for name, c, b in (("frame_level", cfg, batch), ("class_default", cd, cdb)):
        tr = Trainer(c, synth_state_dict(c, 0, duration_bias=math.log(7.0), duration_weight_scale=0.0), **kw)
        ms = loops(tr, b, a.steps, a.warmup)
        res[f"{name}_ms_per_step"], res[f"{name}_ms_all"] = min(ms), [round(m, 3) for m in ms]
        del tr
    F = cfg.variance_filter_size
    res["ops_phone_rows"] = op_times(a.precision, B, L, F)
    res["ops_frame_rows"] = op_times(a.precision, B, T, F)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
