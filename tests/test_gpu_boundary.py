"""Boundary behaviour on the GPU (`-m gpu`): caller-owned workspace (fs2_workspace_bytes / fs2_set_workspace),
the data-parallel aids (zeroed pad rows in the mel store, global-pad frame count) and the host mirror's argument checks."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict
from oracle import oracle_cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    base = dict(n_phones=40, encoder_hidden=128, decoder_hidden=128, encoder_head=2, decoder_head=2, encoder_layers=2,
                decoder_layers=2, encoder_kernel_sizes=[5, 9], decoder_kernel_sizes=[9, 3], encoder_conv_filter_size=256,
                decoder_conv_filter_size=256, encoder_depthwise_conv=False, decoder_depthwise_conv=True,
                variance_filter_size=128, variance_nlayers=[2, 2, 2], duration_filter_size=128)
    base.update(kw)
    return Fs2Config(**base)


def _case(B=4, L=24, lengths=(24, 17, 9, 3), seed=5, **cfgkw):
    cfg = _cfg(**cfgkw)
    sd = synth_state_dict(cfg, seed, randomize_norm=True, duration_bias=1.3)
    inp = synth_inputs(cfg, B, L, seed=seed + 1, lengths=list(lengths))
    batch = {"phones": torch.from_numpy(inp["phones"]), "speaker": torch.from_numpy(inp["speaker"])}
    return cfg, sd, inp, batch


def _model(cfg, sd, precision="fp32", **kw):
    from lightningfastspeech2_amd.model import Engine, FastSpeech2
    m = FastSpeech2(cfg, sd, precision=precision, device="cuda:0")
    if kw:
        m.engine = Engine(cfg, sd, precision=precision, device="cuda:0", **kw)
    return m


def test_caller_workspace_matches_engine_arenas_bitwise():
    """The same forward out of torch-allocated workspace (the default of the host mirror) and out of the engine's own
    hipMalloc arenas: bit-equal; and a too-small caller buffer is refused with the needed size, not overrun."""
    cfg, sd, inp, batch = _case()
    a = _model(cfg, sd, "bf16")                       # torch workspace
    b = _model(cfg, sd, "bf16", torch_workspace=False)  # engine arenas
    oa, ob = a(batch, inference=True), b(batch, inference=True)
    assert a.engine._ws_persist is not None and b.engine._ws_persist is None
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    pb, sb = a.engine.workspace_bytes(4, 24, int(oa["mel"].shape[1]))
    pb0, sb0 = a.engine.workspace_bytes(4, 24, 0)
    assert pb == pb0 and sb >= sb0 > 0
    small = torch.empty(4096, dtype=torch.uint8, device="cuda:0")
    lib = _lib.load()
    st = lib.fs2_set_workspace(a.engine.handle, small, small.numel(), small, small.numel())
    assert st == 0
    a.engine.torch_workspace = False  # stop the mirror from replacing it
    with pytest.raises(RuntimeError, match="workspace too small"):
        a(batch, inference=True)
    assert lib.fs2_set_workspace(a.engine.handle, None, 0, None, 0) == 0
    oc = a(batch, inference=True)
    assert torch.equal(oc["mel"], ob["mel"])


def test_zero_pad_mel_only_touches_pad_rows():
    cfg, sd, inp, batch = _case()
    m = _model(cfg, sd, "fp32")
    ref = m(batch, inference=True)
    m.engine.set_zero_pad_mel(True)
    out = m(batch, inference=True)
    pad = ref["tgt_mask"]
    assert pad.any() and torch.equal(out["mel"][~pad], ref["mel"][~pad])
    assert not out["mel"][pad].any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_global_pad_shard_equals_whole_batch(precision):
    """SURVEY 8e global-pad mode on the engine: a shard that keeps the batch's phone length and is padded to the whole
    batch's frame count (frames_hook -> fs2_set_frames) reproduces its rows of the whole-batch run bit for bit."""
    cfg, sd, inp, batch = _case(B=5, L=24, lengths=(11, 24, 9, 16, 3))
    m = _model(cfg, sd, precision)
    whole = m(batch, inference=True)
    T = int(whole["mel"].shape[1])
    for lo, hi in ((0, 1), (2, 5)):
        sh = {k: v[lo:hi] for k, v in batch.items()}
        out = m.forward(sh, True, frames_hook=lambda t: T)
        assert out["mel"].shape[1] == T
        for k in ("mel", "tgt_mask", "duration_rounded", "variances_pitch"):
            assert torch.equal(out[k], whole[k][lo:hi]), (k, lo)
    with pytest.raises(RuntimeError, match="can only pad"):
        m.forward(batch, True, frames_hook=lambda t: t - 1)


def test_forced_durations_shape_is_checked():
    """a duration target whose shape does not match phones must raise, never be read out of bounds."""
    cfg, sd, inp, batch = _case()
    m = _model(cfg, sd, "fp32")
    ref = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"])
    d = ref["duration_rounded"]
    with pytest.raises(ValueError, match="durations must be"):
        m.forward(batch, force_durations=d[:, :-3])
    wide = torch.nn.functional.pad(d, (0, 4))
    out = m.forward(batch, force_durations=wide)  # zero-padded surplus is harmless
    assert torch.equal(out["tgt_mask"].cpu(), ref["tgt_mask"])
    wide[0, -1] = 2
    with pytest.raises(ValueError, match="non-zero entries beyond"):
        m.forward(batch, force_durations=wide)


def test_priors_may_arrive_as_device_tensors():
    """generate_from_text puts priors in the batch as tensors on the model's device (generator.py:131-146)."""
    stats = {v: {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0} for v in ("pitch", "energy", "snr")}
    stats.update({"pitch_prior": {"min": -2.0, "max": 2.0}, "energy_prior": {"min": -2.0, "max": 2.0}})
    cfg, sd, inp, batch = _case(priors=["pitch", "energy"], stats=stats)
    m = _model(cfg, sd, "fp32")
    pr = {"priors_pitch": np.array([0.1, -0.4, 1.2, 0.0], np.float32), "priors_energy": np.array([-1.0, 0.3, 0.2, 2.0], np.float32)}
    a = m({**batch, **pr}, inference=True)
    b = m({**batch, **{k: torch.from_numpy(v).to("cuda:0") for k, v in pr.items()}}, inference=True)
    assert torch.equal(a["mel"], b["mel"])
    ref = oracle_cpu.forward(sd, cfg, inp["phones"], inp["speaker"], priors=pr)
    assert float((a["mel"].cpu() - ref["mel"]).abs().max()) <= 1e-3


def test_forward_pipeline_is_bit_identical_and_ordered():
    """model.pipeline(n) (r04): n forwards in flight on n engine replicas / HIP streams / host threads.  Every batch's outputs equal
    the synchronous model(batch)'s bit for bit and come back in submission order, for ragged batches of different shapes."""
    cfg, sd, inp, batch = _case()
    m = _model(cfg, sd, "bf16")
    rs = np.random.RandomState(3)
    batches = []
    for i in range(7):
        B = int(rs.randint(1, 5))
        L = int(rs.randint(5, 25))
        lens = sorted((int(rs.randint(1, L + 1)) for _ in range(B)), reverse=True)
        lens[0] = L
        x = synth_inputs(cfg, B, L, seed=50 + i, lengths=lens)
        batches.append({"phones": torch.from_numpy(x["phones"]).cuda(), "speaker": torch.from_numpy(x["speaker"]).cuda()})
    want = [m(b, inference=True) for b in batches]
    for n in (1, 2, 3):
        pipe = m.pipeline(n)
        got = []
        for b in batches:
            got += pipe.submit(b)
        got += pipe.drain()
        pipe.close()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.keys() == w.keys()
            for k in w:
                assert torch.equal(g[k], w[k]), (n, k)


def test_forward_pipeline_with_the_host_boundary_inside_is_bit_identical():
    """model.pipeline(n, host_outputs=("mel", "tgt_mask")) (r06; the consumer modelled: generator.py:158-165, `mel[i][~tgt_mask[i]].cpu()`):
    pinned HOST batches in, the named outputs back as pinned host tensors whose device-to-host copies ran on a copy stream under the next
    forward.  Every batch: the same bytes as model(batch)[key].cpu(), in submission order, the other outputs still device tensors; results
    are consumed at hand-over (a host output's ring slot is reused four runs of its replica later)."""
    cfg, sd, inp, batch = _case()
    m = _model(cfg, sd, "bf16")
    rs = np.random.RandomState(5)
    batches = []
    for i in range(11):
        B = int(rs.randint(1, 5))
        L = int(rs.randint(5, 25))
        lens = sorted((int(rs.randint(1, L + 1)) for _ in range(B)), reverse=True)
        lens[0] = L
        x = synth_inputs(cfg, B, L, seed=90 + i, lengths=lens)
        batches.append({"phones": torch.from_numpy(x["phones"]).pin_memory(), "speaker": torch.from_numpy(x["speaker"]).pin_memory()})
    want = [{k: v.cpu() for k, v in m(b, inference=True).items()} for b in batches]
    for n in (1, 2, 3):
        pipe = m.pipeline(n, host_outputs=("mel", "tgt_mask"))
        got = []

        def take(outs):
            for o in outs:
                assert not o["mel"].is_cuda and o["mel"].is_pinned() and not o["tgt_mask"].is_cuda
                assert o["duration_rounded"].is_cuda
                got.append({k: v.cpu().clone() for k, v in o.items()})  # consumed at hand-over
        for b in batches:
            take(pipe.submit(b))
        take(pipe.drain())
        pipe.close()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.keys() == w.keys()
            for k in w:
                assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), (n, k)


def test_two_engines_with_different_tuning_run_concurrently():
    """The kernel-selection switches are per engine (fs2_set_tuning), not process state: two replicas of one model -
    one on the defaults, one with the GEMM and predictor-tail forms switched to their other, bit-identical kernels - driven
    by two host threads on two streams at once give the same bits as the synchronous default engine, batch for batch; and a
    thread-level fs2_op_set_gemm_variant in between touches neither."""
    import concurrent.futures as cf
    from lightningfastspeech2_amd.config import preset
    cfg = preset("c2")
    sd = synth_state_dict(cfg, 3, randomize_norm=True, duration_bias=1.5)
    m = _model(cfg, sd, "bf16")
    rs = np.random.RandomState(7)
    batches = []
    for i in range(6):
        B, L = int(rs.randint(2, 6)), int(rs.randint(30, 90))
        lens = sorted((int(rs.randint(1, L + 1)) for _ in range(B)), reverse=True)
        lens[0] = L
        x = synth_inputs(cfg, B, L, seed=70 + i, lengths=lens)
        batches.append({"phones": torch.from_numpy(x["phones"]).cuda(), "speaker": torch.from_numpy(x["speaker"]).cuda()})
    want = [m(b, inference=True) for b in batches]
    torch.cuda.synchronize()
    a, b = m.replicate(), m.replicate()
    for knob in (1400, 1320, 220, 200):   # slab-kernel in-projection, stand-alone bucket_embed, no persistent GEMM, plain tile order
        b.engine.set_tuning(knob)
    assert _lib.load().fs2_op_set_gemm_variant(1204) == 0   # this thread's operator-level switch: no engine reads it
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def run(model, stream):
        out = []
        with torch.cuda.stream(stream):
            for bt in batches:
                out.append(model(bt, inference=True))
            stream.synchronize()
        return out
    try:
        with cf.ThreadPoolExecutor(max_workers=2) as pool:
            fa, fb = pool.submit(run, a, streams[0]), pool.submit(run, b, streams[1])
            ga, gb = fa.result(), fb.result()
    finally:
        _lib.load().fs2_op_set_gemm_variant(1203)
    for i, w in enumerate(want):
        for k in w:
            assert torch.equal(ga[i][k], w[k]), ("defaults", i, k)
            assert torch.equal(gb[i][k], w[k]), ("switched", i, k)


def test_engine_clone_shares_weights_and_outlives_its_parent():
    """fs2_clone: a second engine over the same device weights; the weights are freed with the LAST holder, so a clone keeps working
    after its parent is destroyed, and gives the parent's results bit for bit."""
    cfg, sd, inp, batch = _case()
    m = _model(cfg, sd, "bf16")
    want = m(batch, inference=True)
    before = torch.cuda.memory_allocated()
    r = m.replicate()
    got = r(batch, inference=True)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    m.engine.close()            # parent gone: the clone still holds the weight blocks
    again = r(batch, inference=True)
    assert torch.equal(again["mel"], want["mel"])
    del before


def test_two_rank_bench_rehearsal_over_gloo():
    """bench.py's multi-rank control flow (shape agreement once, sync-free gathers with zeroed pad rows, drain, max over
    ranks) with both ranks on this box's one GPU over gloo - the RCCL run itself needs the 8-GPU node."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, FS2_BENCH_BACKEND="gloo", FS2_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--config", "ref-default", "--batch", "4", "--phones", "32"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 8 and line["value"] > 0
    assert line["config"]["frames_per_utterance"] == 32 * 6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_rccl_branch_runs_at_world_size_one():
    """The backend == "nccl" paths (= RCCL on ROCm) of dist.py on the hardware that exists: librccl loads, the process group
    comes up with device_id=, the mel gather queues on the collective stream and MelGather.wait orders the caller's stream
    behind it, global_frames / all_reduce_gradients run - before an 8-GPU node ever sees them.  In a child process: a process
    group in the pytest process would outlive the test."""
    code = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["FS2_ROOT"])
from lightningfastspeech2_amd.dist import gather_mels_async, global_frames, all_reduce_gradients, forward_sharded, collective_device
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
assert dist.get_backend() == "nccl"
assert collective_device(None, None) == torch.device("cuda", 0)           # a host-side batch still gets device control tensors
mel = torch.randn(3, 40, 80, device="cuda")
mask = torch.zeros(3, 40, dtype=torch.bool, device="cuda"); mask[1, 25:] = True; mask[2, 10:] = True
mel[mask] = 0
g = gather_mels_async(mel, mask, zeroed=True)                               # general path: exchanges (B_r, T) first
all_mel, frames = g.wait()
torch.cuda.synchronize()
assert torch.equal(all_mel, mel) and frames.tolist() == [40, 25, 10]
g2 = gather_mels_async(mel, mask, shapes=([3], 40), zeroed=True)            # sync-free path (bench.py's steady state)
all2, fr2 = g2.wait(); torch.cuda.synchronize()
assert torch.equal(all2, mel) and fr2.tolist() == [40, 25, 10]
assert global_frames(123, torch.device("cuda", 0)) == 123
flat = torch.arange(1000, dtype=torch.float32, device="cuda")
all_reduce_gradients(flat, bucket_bytes=1024)                               # four buckets
works = all_reduce_gradients(flat, bucket_bytes=2048, async_op=True)
for w in works: w.wait()
torch.cuda.synchronize()
assert torch.equal(flat.cpu(), torch.arange(1000, dtype=torch.float32))
out = forward_sharded(lambda b: {"mel": mel[:b["phones"].shape[0]], "tgt_mask": mask[:b["phones"].shape[0]]},
                      {"phones": torch.ones(3, 5, dtype=torch.long), "speaker": torch.zeros(3, 256)}, n_mels=80)
assert out[0].shape == (3, 40, 80) and out[0].is_cuda
dist.destroy_process_group()
print("RCCL-OK")
'''
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), FS2_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL-OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_bench_under_torchrun_over_rccl_one_rank():
    """bench.py exactly as the driver launches it for N > 1 (torch.distributed.run, one rank per GPU, backend nccl), with the
    multi-rank path forced at world size 1 (FS2_BENCH_FORCE_DIST): init with device_id=, shape agreement, gathers in flight under
    the next forward, drain, closing barrier, max over ranks."""
    env = dict(os.environ, FS2_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "ref-default", "--batch", "4", "--phones", "32", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and "RCCL" in line["config"]["parallelism"]
    # the evidence a SCALE line needs to be checkable: the ranks RCCL really connected, per-rank step times and frames, gather bytes
    d = line["dist"]
    assert d["backend"] == "nccl" and d["world_size"] == 1 and d["ranks_seen"] == [0] and d["forced_single_rank"]
    assert len(d["per_rank_ms_per_step"]) == 1 and d["per_rank_ms_per_step"][0] > 0
    T = line["config"]["frames_per_utterance"]
    assert d["gather_bytes_per_rank"] == 4 * T * 80 * 4 + 4 * 8 and d["per_rank_frames_per_step"] == [4 * T]
    assert d["rccl_version"] and isinstance(d["gather_ms_exposed"], float)


def test_forced_dist_line_agrees_with_the_plain_line():
    """at N = 1 the multi-rank path (process group over RCCL, asynchronous mel gather under the next forward,
    closing barrier) must cost the step nothing measurable - its line agrees with the plain single-GPU line on the headline
    workload.  Best of two runs each (box noise between two processes is ~1-2 %).  Bar 7 %: with two forwards in flight the GPU has no
    idle left to hide the gather's 15.7 MB device copy + its four small launches under (measured r04: 1.875 vs 1.944 ms, 3.7 %; with one
    forward in flight both lines read 2.05 ms) - the line's own dist.gather_ms_exposed says how much that is."""
    def run(force):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
        if force:
            env["FS2_BENCH_FORCE_DIST"] = "1"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "30", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-parity",
               "--no-train"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    plain, forced = [run(False), run(False)], [run(True), run(True)]
    a, b = min(l["ms_per_step"] for l in plain), min(l["ms_per_step"] for l in forced)
    assert forced[0]["dist"]["ranks_seen"] == [0] and "dist" not in plain[0]
    # (7 %: the gather's ~4 % plus what two processes on one box differ by; the test failed once at 5 % and passed on the next box)
    assert abs(b - a) <= 0.07 * a, (a, b, forced[0]["dist"])
    assert min(l["dist"]["gather_ms_exposed"] for l in forced) <= 0.07 * a


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run times exactly --steps steps and prints the headline line without the --full side measurements;
    --dump-outputs writes the last timed step's outputs as float32 .npy files, the same ones on a second run with the same
    arguments (seeded inputs, a forward without atomics)."""
    def run(d):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--config", "ref-default",
               "--batch", "4", "--phones", "32", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    line = run(tmp_path / "a")
    T = 32 * 6
    assert line["steps"] == 4 and line["warmup"] == 1 and line["config"]["frames_per_utterance"] == T
    assert line["unit"] == "mel-frames/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 4 * T) <= 1e-6 * 4 * T   # value = frames per step / one step's time
    for k in ("roofline", "north_star_attention", "encoder_mha_block", "gpu_ms_per_step", "value_incl_pcie", "parity", "training_step",
              "cpu_baseline", "dist"):
        assert k not in line, k
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert {"mel", "tgt_mask", "src_mask", "duration_rounded", "duration_prediction"} <= set(a)
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["mel"].shape == (4, T, 80) and np.isfinite(a["mel"]).all() and float(np.abs(a["mel"]).max()) > 0
    assert not a["tgt_mask"].any() and (a["duration_rounded"] == 6).all()
    run(tmp_path / "b")
    for k, v in a.items():
        assert np.array_equal(np.load(tmp_path / "b" / f"{k}.npy"), v), k
