#!/usr/bin/env python
"""A/B of the slab GEMM's K loop per launch class: two weight stages (knob 240) against the lead-2 loop (242), interleaved in one
process, HIP-event timed, at the C2 shapes of the forward (FS2-27M, B = 32, L = 256, T = 1536) and at the K = 256 / k = 3
LayerNorm launches of other configs.
    python tools/bench_slab_lead.py [--rounds R] [--reps N] [--flush MB] [--only SUBSTR]
A round times `reps` back-to-back launches under each knob; per class the table gives median and min over the rounds, the spread
(max - min) of the "off" rounds, and whether the lead-2 median is lower by more than that spread.  Both forms store the same bits
(tests/test_gpu_slab_lead.py); the first round's outputs are compared here as well."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightningfastspeech2_amd import _lib  # noqa: E402

lib = _lib.load()
DEV = "cuda:0"
BF16 = _lib.FS2_BF16

# name, M, N, Cin, taps, S, kind (plain / ln), relu, residual
CLASSES = [
    ("enc conv1 k9 +relu", 8192, 1024, 256, 9, 256, "plain", True, False),
    ("enc in-proj K256", 8192, 768, 256, 1, 256, "plain", False, False),
    ("dec conv2 K1024 +res+LN", 49152, 256, 1024, 1, 1536, "ln", False, True),
    ("dec out-proj K256 +res+LN", 49152, 256, 256, 1, 1536, "ln", False, True),
    ("enc conv2 K1024 +res+LN", 8192, 256, 1024, 1, 256, "ln", False, True),
    ("enc out-proj K256 +res+LN", 8192, 256, 256, 1, 256, "ln", False, True),
    ("k3 +relu+LN, 8192 rows", 8192, 256, 256, 3, 256, "ln", True, False),
    ("k3 +relu+LN, 49152 rows", 49152, 256, 256, 3, 1536, "ln", True, False),
    ("dec conv1 k9 +relu (256-row tiles: no lead-2 form)", 49152, 1024, 256, 9, 1536, "plain", True, False),
]


def make(M, N, Cin, taps, S, kind, relu, res):
    g = torch.Generator(device=DEV).manual_seed(M + N + Cin + taps)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    x = r(M, Cin).to(torch.bfloat16)
    w = (r(N, taps * Cin) * (taps * Cin) ** -0.5).to(torch.bfloat16)
    b = r(N)
    c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    if kind == "plain":
        return c, lambda st: lib.fs2_op_gemm(BF16, BF16, x, w, b, c, M, N, Cin, taps, S, int(relu), st)
    rr = r(M, N).to(torch.bfloat16) if res else None
    ga, be = r(N), r(N)
    tmp = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    return c, lambda st: lib.fs2_op_gemm_ln(BF16, x, w, b, rr, ga, be, None, 0.0, None, None, c, tmp, M, N, Cin, taps, S, int(relu), st)


def timed(fn, reps, flush):
    st = torch.cuda.current_stream()
    if flush is not None:
        tot = 0.0
        for _ in range(reps):
            flush.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn(st) == 0
            e1.record()
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / reps * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert fn(st) == 0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--flush", type=int, default=0, help="MB of unrelated memory touched before every launch (cold caches, as inside a forward); 0 = back-to-back")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    flush = torch.zeros(a.flush * (1 << 20) // 4, device=DEV) if a.flush else None
    print(f"# rounds {a.rounds}, reps {a.reps}, flush {a.flush} MB; times in us; off = knob 240, on = knob 242")
    print("| launch class | off median | off min | off spread | on median | on min | on - off (median) | faster by more than the off spread |")
    print("|---|---|---|---|---|---|---|---|")
    try:
        for (name, M, N, Cin, taps, S, kind, relu, res) in CLASSES:
            if a.only and a.only not in name:
                continue
            c, fn = make(M, N, Cin, taps, S, kind, relu, res)
            t = {240: [], 242: []}
            outs = {}
            for knob in (240, 242):  # warm both forms, keep their bits
                assert lib.fs2_op_set_gemm_variant(knob) == 0
                timed(fn, 3, None)
                outs[knob] = c.clone()
            same = torch.equal(outs[240], outs[242])
            for _ in range(a.rounds):
                for knob in (240, 242):
                    lib.fs2_op_set_gemm_variant(knob)
                    t[knob].append(timed(fn, a.reps, flush))
            off, on = t[240], t[242]
            spread = max(off) - min(off)
            d = statistics.median(on) - statistics.median(off)
            print(f"| {name} | {statistics.median(off):.1f} | {min(off):.1f} | {spread:.1f} | {statistics.median(on):.1f} | {min(on):.1f} | "
                  f"{d:+.1f} | {'yes' if -d > spread else 'no'} |" + ("" if same else "  BITS DIFFER"), flush=True)
    finally:
        lib.fs2_op_set_gemm_variant(241)


if __name__ == "__main__":
    main()
