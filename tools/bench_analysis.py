#!/usr/bin/env python
"""Benchmark of the analysis front end (waveform -> log-mel + energy, fs2_mel_run) at the mel forward's own output size:
B utterances x S samples of noise resident in HBM -> (B, 1 + S / hop, n_mels) log-mel and (B, S / hop) energy.

    python tools/bench_analysis.py [--batch 32 --samples 393216 --steps 20 --loops 5 --warmup 3 --no-cpu --snr --pitch --cwt]

One process, the fastest of --loops timed loops (device events around --steps calls) each:
  * the whole operator (peak + STFT / mel + energy launches) and the STFT / mel launch alone;
  * its share of the fp32 MFMA rate MI355X_MICROARCH gives as measured (155 TFLOP/s), from the algorithmic FLOPs of the trimmed
    DFT and the mel product, and which limit it is on: the larger of FLOPs / 155 TF, HBM bytes / 6.29 TB/s and the DFT table
    every workgroup streams from L2 / 17 TB/s;
  * next to it the CPU recipe it replaces on this box: torch.stft + matmul + clamp + log10 in float32 on 16 threads.
With --snr, in the same process after the mel figures: the windowed WADA estimate (fs2_mel_snr: peak + statistic launches) on the
same batch, its HBM floor - the waveform read twice, once for the peak and once for the statistic - and this project's own numpy
loop of the same definition on --snr-cpu-rows utterances of the batch (one window at a time, as the reference's loop goes), scaled to
the batch.  The WADA table is an argument of the operator (the project ships none): --wada-table names an .npy, or an .npz with a
"wada_table" array (default: the test fixture).
With --pitch, in the same process: the F0 tracker (fs2_mel_pitch, one launch) on a harmonic glide with noise of the same batch size,
the rate of its hot loop - sample-lag pairs (x[j] - x[j + tau])^2 per second, per-hop partials counted once, 3 FLOP a pair against
the 157.3 TFLOP/s the fp32 vector units have on paper - and this project's own numpy float32 restatement of the same definition
(per-hop partials, one lag at a time) on --cpu-threads threads, the fastest of --loops loops each.
With --cwt, in the same process: the CWT decomposition (fs2_op_cwt_decompose, one launch) on --batch contours of 1536 entries (frame
level) and of 256 (phone level), against two floors - the HBM floor of two reads of the contour plus the writes of original, signal
and the 10-scale spectrogram, and the launch floor, measured as the same launch with every count 0 (each workgroup returns at once) -
the rate of its fp64 multiply-adds (taps that fall inside the utterance), and this project's own numpy restatement of the same
definition (np.convolve per scale, a row per thread) on --cpu-threads threads.
Prints ONE JSON line.  No GPU, no figure: the tool fails without a device.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.analysis import MelAnalyzer

VALU_F32 = 157.3e12  # the fp32 vector rate on paper (packed FMA on every lane of 256 CUs at 2.4 GHz)
MFMA_F32, HBM, L2 = 155e12, 6.29e12, 17e12  # measured rates (fp32 MFMA, float4 copy, rows shared by every workgroup from L2)


def cpu_recipe(x, basis, n_fft, hop, win, clip):
    mag = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win), center=True, pad_mode="constant",
                     return_complex=True).abs()
    return torch.log10(torch.clamp(torch.matmul(basis, mag), min=clip))


def wada_numpy(x, win, hop, g):
    """the definition of include/fs2.h, window by window, on one peak-normalised float32 utterance"""
    n = len(x)
    out = np.full(-(-n // hop), np.nan, np.float32)
    for t in range(len(out)):
        seg = np.abs(x[t * hop:min(t * hop + win, n)])
        if not seg.any() or not (seg * seg).any():
            continue
        a = np.maximum(seg, np.float32(1e-20))
        v3 = np.log(max(1e-20, float(a.mean(dtype=np.float64)))) - float(np.log(a).mean(dtype=np.float64))
        below = np.nonzero(g < v3)[0]
        if len(below) and below[-1] < len(g) - 1:
            i = below[-1]
            o = i + (v3 - g[i]) / (g[i + 1] - g[i])
            if o < len(g) - 1:
                out[t] = o
    return out


def yin_numpy(x, win, hop, sr, tau_min, tau_max, threshold):
    """the definition of include/fs2.h "F0 tracking" on one float32 utterance (win % hop == 0): per-hop partial sums one lag at a
    time, a frame's win / hop added left to right, everything in float32 -> (f0 (Tf,), voiced (Tf,))"""
    n, r, nl = len(x), win // hop, tau_max + 2
    tf = 1 + n // hop
    blocks = tf + r - 1
    xp = np.zeros(blocks * hop + nl, np.float32)
    xp[win // 2:win // 2 + n] = x
    a = xp[:blocks * hop]
    part = np.empty((blocks, nl), np.float32)
    for tau in range(nl):
        diff = a - xp[tau:tau + blocks * hop]
        part[:, tau] = (diff * diff).reshape(blocks, hop).sum(axis=1)
    d = part[:tf].copy()
    for i in range(1, r):
        d += part[i:i + tf]
    cum = np.cumsum(d[:, 1:], axis=1, dtype=np.float32)
    cm = np.ones_like(d)
    np.divide(d[:, 1:] * np.arange(1, nl, dtype=np.float32), cum, out=cm[:, 1:], where=cum != 0)
    below = cm[:, tau_min:tau_max + 1] < threshold
    voiced = below.any(axis=1)
    tau = tau_min + below.argmax(axis=1)
    rows = np.arange(tf)
    while True:  # the forward walk, on all frames that still step
        step = voiced & (tau + 1 <= tau_max) & (cm[rows, np.minimum(tau + 1, nl - 1)] < cm[rows, tau])
        if not step.any():
            break
        tau = tau + step
    p, q, s = cm[rows, tau - 1], cm[rows, tau], cm[rows, tau + 1]
    curv = p - 2 * q + s
    delta = np.where(curv > 0, np.clip((p - s) / np.where(curv > 0, 2 * curv, 1), -0.5, 0.5), 0)
    return np.where(voiced, sr / (tau + delta), 0).astype(np.float32), voiced


def cwt_numpy(v, n_scales=10, tau=0.2833425):
    """the definition of include/fs2.h "CWT and log variance targets" on one float32 contour -> the (n, n_scales) spectrogram"""
    s = np.where(v == 0, np.float32(1e-7), v)
    s = np.log(s.astype(np.float64)).astype(np.float32)
    x = (s - s.mean()) / (s.std() + np.float32(1e-7))
    out = np.empty((len(v), n_scales), np.float32)
    for i in range(1, n_scales + 1):
        w = 2 ** (i + 1) * tau
        N = min(10 * w, len(v))
        vec = np.arange(0, N) - (N - 1.0) / 2
        r = 2 / (np.sqrt(3 * w) * np.pi ** 0.25) * (1 - vec ** 2 / w ** 2) * np.exp(-vec ** 2 / (2 * w ** 2))
        full = np.convolve(x, r[::-1])
        start = (len(full) - len(v)) // 2
        out[:, i - 1] = full[start:start + len(v)] * (i + 2.5) ** (-5 / 2)
    return out


def cwt_taps(n, n_scales=10, tau=0.2833425):
    """multiply-adds of one utterance: per scale and output, the taps that fall inside [0, n)"""
    total = 0
    for i in range(1, n_scales + 1):
        M = int(np.ceil(min(10 * 2 ** (i + 1) * tau, n)))
        j = np.arange(n)[:, None] - M // 2 + np.arange(M)[None, :]
        total += int(((j >= 0) & (j < n)).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=393216)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--snr", action="store_true")
    ap.add_argument("--snr-cpu-rows", type=int, default=2)
    ap.add_argument("--pitch", action="store_true")
    ap.add_argument("--pitch-cpu-rows", type=int, default=0, help="rows the numpy restatement runs (0: the whole batch); scaled to the batch")
    ap.add_argument("--cwt", action="store_true")
    ap.add_argument("--wada-table", default=os.path.join(ROOT, "tests", "golden", "frontend_targets.npz"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_analysis needs an MI355X: no figure without a device")
    dev = torch.device("cuda:0")
    an = MelAnalyzer(device=dev)
    lib, B, S, hop, nm = an.lib, a.batch, a.samples, an.hop_length, an.n_mels
    T, Te = 1 + S // hop, -(-S // hop)
    wav = (0.3 * torch.randn(B, S, generator=torch.Generator().manual_seed(0))).to(dev)
    lengths = torch.full((B,), S, dtype=torch.int32, device=dev)
    mel = torch.empty(B, T, nm, device=dev)
    energy = torch.empty(B, Te, device=dev)
    mf, ef = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    need = lib.fs2_mel_ws_bytes(an.handle, B, S)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream()

    def run(full):
        st = lib.fs2_mel_run(an.handle, wav, lengths, B, S, int(full), mel, T, energy if full else None, Te, mf, ef, ws, need, stream)
        assert st == 0, lib.fs2_mel_last_error(an.handle)

    def fastest(full, run=run):
        for _ in range(a.warmup):
            run(full)
        ms = []
        for _ in range(a.loops):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                run(full)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.steps)
        return min(ms), ms

    stft_ms, stft_loops = fastest(False)
    full_ms, full_loops = fastest(True)
    assert bool(torch.isfinite(mel).all()) and mf.tolist() == [T] * B
    used = int(np.count_nonzero(an.mel_basis.any(axis=0)))
    first, cols = C.c_int32(), C.c_int32()
    assert lib.fs2_mel_used_bins(an.handle, C.byref(first), C.byref(cols)) == 0
    frames = B * T
    flops = frames * (2.0 * an.n_fft * 2 * used + 2.0 * used * nm)
    hbm_bytes = 4.0 * (B * S + frames * nm)
    tiles = B * -(-T // an.tile_frames)
    l2_bytes = tiles * 4.0 * an.n_fft * 2 * cols.value
    bounds = {"fp32_mfma": flops / MFMA_F32 * 1e3, "hbm": hbm_bytes / HBM * 1e3, "l2_table": l2_bytes / L2 * 1e3}
    limit = max(bounds, key=bounds.get)
    out = {"tool": "bench_analysis", "batch": B, "samples": S, "frames": frames, "n_fft": an.n_fft, "hop": hop, "n_mels": nm,
           "tile_frames": an.tile_frames, "dft_bins": used, "dft_columns": 2 * cols.value,
           "operator_ms": round(full_ms, 4), "operator_loops_ms": [round(x, 4) for x in full_loops],
           "stft_mel_ms": round(stft_ms, 4), "stft_mel_loops_ms": [round(x, 4) for x in stft_loops],
           "gflop": round(flops / 1e9, 2), "stft_mel_tflops": round(flops / stft_ms / 1e9, 2),
           "share_of_fp32_mfma_155tf": round(bounds["fp32_mfma"] / stft_ms, 4),
           "bounds_ms": {k: round(v, 4) for k, v in bounds.items()}, "limit": limit,
           "share_of_limit": round(bounds[limit] / stft_ms, 4),
           "audio_seconds_per_second": round(B * S / an.sampling_rate / (full_ms / 1e3), 1),
           "steps": a.steps, "loops": a.loops, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    if not a.no_cpu:
        torch.set_num_threads(a.cpu_threads)
        x, basis = wav.cpu(), torch.from_numpy(an.mel_basis)
        cpu_recipe(x[:2], basis, an.n_fft, hop, an.win_length, an.clip)
        cpu = []
        for _ in range(a.loops):
            t0 = time.perf_counter()
            ref = cpu_recipe(x, basis, an.n_fft, hop, an.win_length, an.clip)
            cpu.append((time.perf_counter() - t0) * 1e3)
        run(False)
        torch.cuda.synchronize()
        out.update({"cpu_recipe_ms": round(min(cpu), 2), "cpu_threads": a.cpu_threads, "cpu_loops_ms": [round(v, 2) for v in cpu],
                    "speedup_vs_cpu_recipe": round(min(cpu) / full_ms, 1),
                    "max_abs_log10_vs_cpu_recipe": float((mel.cpu() - ref.permute(0, 2, 1)).abs().max())})
    if a.snr:
        table = np.load(a.wada_table)
        table = np.asarray(table["wada_table"] if hasattr(table, "files") else table, np.float64)
        an.set_wada_table(table)
        snr = torch.empty(B, Te, device=dev)
        sf = torch.empty(B, dtype=torch.int32, device=dev)

        def run_snr(_full=True):
            st = lib.fs2_mel_snr(an.handle, wav, lengths, B, S, 1, snr, Te, sf, ws, need, stream)
            assert st == 0, lib.fs2_mel_last_error(an.handle)

        snr_ms, snr_loops = fastest(True, run_snr)
        assert sf.tolist() == [Te] * B
        floor_ms = 2 * 4.0 * B * S / HBM * 1e3
        out.update({"snr_ms": round(snr_ms, 4), "snr_loops_ms": [round(x, 4) for x in snr_loops], "snr_windows": B * Te,
                    "snr_hbm_floor_ms": round(floor_ms, 4), "snr_ratio_to_floor": round(snr_ms / floor_ms, 2),
                    "snr_nan_share": round(float(torch.isnan(snr).float().mean()), 4)})
        if not a.no_cpu:
            rows = max(1, min(a.snr_cpu_rows, B))
            x = wav[:rows].cpu().numpy()
            x = x / np.abs(x).max(axis=1, keepdims=True)
            t0 = time.perf_counter()
            ref = np.stack([wada_numpy(r, an.win_length, hop, table) for r in x])
            loop_ms = (time.perf_counter() - t0) * 1e3
            got = snr[:rows].cpu().numpy()
            both = ~np.isnan(ref) & ~np.isnan(got)
            out.update({"snr_numpy_loop_rows": rows, "snr_numpy_loop_ms": round(loop_ms, 1),
                        "snr_numpy_loop_ms_scaled_to_batch": round(loop_ms * B / rows, 1),
                        "snr_speedup_vs_numpy_loop": round(loop_ms * B / rows / snr_ms, 0),
                        "snr_max_abs_db_vs_numpy_loop": float(np.abs(ref[both] - got[both]).max()) if both.any() else None})
    if a.pitch:
        sr, floor, ceil, thr = an.sampling_rate, 71.0, 800.0, 0.1
        lo, hi = C.c_int32(), C.c_int32()
        assert lib.fs2_mel_pitch_lags(an.handle, sr, floor, ceil, C.byref(lo), C.byref(hi)) == 0
        nl, tile = hi.value + 2, lib.fs2_mel_pitch_tile_frames(an.handle, sr, floor)
        # a harmonic glide 100 -> 400 Hz per row (six harmonics at 1 / k) with the batch's noise 20 dB below it
        phase = 2 * np.pi * torch.cumsum(torch.linspace(100.0, 400.0, S, dtype=torch.float64), 0) / sr
        voice = sum(torch.sin(k * phase) / k for k in range(1, 7)).to(torch.float32).to(dev)
        pwav = (0.5 * voice[None, :] / voice.abs().max() + 0.1 * wav).contiguous()
        f0 = torch.empty(B, T, device=dev)
        dmin = torch.empty(B, T, device=dev)
        ff = torch.empty(B, dtype=torch.int32, device=dev)

        def run_pitch(_full=True):
            st = lib.fs2_mel_pitch(an.handle, pwav, lengths, B, S, sr, floor, ceil, thr, f0, T, ff, dmin, None, 0, stream)
            assert st == 0, lib.fs2_mel_last_error(an.handle)

        pitch_ms, pitch_loops = fastest(True, run_pitch)
        assert ff.tolist() == [T] * B and bool(torch.isfinite(f0).all())
        pairs = float(B) * (T + an.win_length // hop - 1) * hop * nl  # every hop of an utterance once, every lag
        out.update({"pitch_ms": round(pitch_ms, 4), "pitch_loops_ms": [round(x, 4) for x in pitch_loops], "pitch_frames": B * T,
                    "pitch_lags": nl, "pitch_tile_frames": tile, "pitch_form": "direct (x[j] - x[j + tau])^2, fp32 VALU",
                    "pitch_gpairs": round(pairs / 1e9, 2), "pitch_gpairs_per_s": round(pairs / pitch_ms / 1e6, 1),
                    "pitch_share_of_fp32_vector_157tf": round(3.0 * pairs / (pitch_ms / 1e3) / VALU_F32, 4),
                    "pitch_voiced_share": round(float((f0 > 0).float().mean()), 4),
                    "pitch_audio_seconds_per_second": round(B * S / sr / (pitch_ms / 1e3), 1)})
        if not a.no_cpu:
            from concurrent.futures import ThreadPoolExecutor
            rows = B if a.pitch_cpu_rows <= 0 else min(a.pitch_cpu_rows, B)
            x = pwav[:rows].cpu().numpy()
            one = lambda r: yin_numpy(r, an.win_length, hop, sr, lo.value, hi.value, thr)
            cpu = []
            with ThreadPoolExecutor(a.cpu_threads) as pool:  # numpy releases the GIL inside its loops: a row per thread
                for _ in range(a.loops):
                    t0 = time.perf_counter()
                    ref = list(pool.map(one, x))
                    cpu.append((time.perf_counter() - t0) * 1e3 * B / rows)
            got = f0[:rows].cpu().numpy()
            rf0, rv = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
            both = rv & (got > 0)
            out.update({"pitch_numpy_rows": rows, "pitch_numpy_threads": a.cpu_threads, "pitch_numpy_ms": round(min(cpu), 1),
                        "pitch_numpy_loops_ms": [round(v, 1) for v in cpu], "pitch_speedup_vs_numpy": round(min(cpu) / pitch_ms, 0),
                        "pitch_voiced_flags_equal_share": round(float((rv == (got > 0)).mean()), 6),
                        "pitch_max_rel_f0_vs_numpy": float(np.abs(got[both] / rf0[both] - 1).max()) if both.any() else None})
    if a.cwt:
        from concurrent.futures import ThreadPoolExecutor
        ns, tau = 10, 0.2833425
        for level, Sc in (("frame", 1536), ("phone", 256)):
            rs = np.random.RandomState(Sc)  # contours shaped like F0: log-normal about 180 Hz, a slow wander plus jitter
            host = (180.0 * np.exp(0.3 * np.sin(np.arange(Sc)[None, :] / 11.0 + rs.uniform(0, 6, (B, 1))) + 0.05 * rs.standard_normal((B, Sc)))).astype(np.float32)
            vals = torch.from_numpy(host).to(dev)
            full, none = torch.full((B,), Sc, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            orig, sig = torch.empty(B, Sc, device=dev), torch.empty(B, Sc, device=dev)
            spec, ms2 = torch.empty(B, Sc, ns, device=dev), torch.empty(B, 2, device=dev)

            def run_cwt(counts):
                assert lib.fs2_op_cwt_decompose(vals, counts, B, Sc, ns, tau, orig, sig, spec, ms2, stream) == 0

            cwt_ms, cwt_loops = fastest(full, run_cwt)
            assert bool(torch.isfinite(spec).all())
            launch_ms, _ = fastest(none, run_cwt)
            floor_ms = 4.0 * B * Sc * (2 + 2 + ns) / HBM * 1e3
            fmas = float(B) * cwt_taps(Sc, ns, tau)
            res = {"entries": Sc, "ms": round(cwt_ms, 4), "loops_ms": [round(x, 4) for x in cwt_loops], "hbm_floor_ms": round(floor_ms, 5),
                   "launch_floor_ms": round(launch_ms, 4), "ratio_to_hbm_floor": round(cwt_ms / floor_ms, 1),
                   "ratio_to_launch_floor": round(cwt_ms / launch_ms, 1), "fp64_fmas": fmas, "fp64_gfma_per_s": round(fmas / cwt_ms / 1e6, 1)}
            if not a.no_cpu:
                cpu = []
                with ThreadPoolExecutor(a.cpu_threads) as pool:  # numpy releases the GIL inside np.convolve: a row per thread
                    for _ in range(a.loops):
                        t0 = time.perf_counter()
                        ref = np.stack(list(pool.map(cwt_numpy, host)))
                        cpu.append((time.perf_counter() - t0) * 1e3)
                run_cwt(full)
                res.update({"numpy_ms": round(min(cpu), 2), "numpy_threads": a.cpu_threads, "numpy_loops_ms": [round(v, 2) for v in cpu],
                            "speedup_vs_numpy": round(min(cpu) / cwt_ms, 0),
                            "max_abs_vs_numpy_over_peak": float(np.abs(spec.cpu().numpy() - ref).max() / np.abs(ref).max())})
            out[f"cwt_{level}"] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
