"""FastDiff on the CPU: the host mirror (names, schedules, noise order, synthetic weights) and the restatement the GPU tests judge the
device by, against what the reference's own FastDiff returned (tests/golden/fastdiff/, tools/gen_golden_fastdiff.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _fastdiff_ref as R
from _fastdiff_ref import fixture, schedule, weights
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd import fastdiff as FD

CASES = ("ragged", "long")
# The float32 restatement and the reference are two float32 evaluations of one function: each lies within the reference's recorded
# distance to float64 (*_err64) of the truth up to the difference in summation order (torch's conv kernels pick their own per
# shape), so they are at most a few of those distances apart.  An indexing error is five orders of magnitude larger.
MARGIN = 4


@functools.lru_cache(maxsize=None)
def ref32():
    return R.FastDiffRef(weights(), torch.float32)


def test_state_dict_spec_is_the_references():
    meta = fixture("ragged")["meta"]
    spec = FD.state_dict_spec(FD.FastDiffConfig())
    assert {k: list(v) for k, v in spec.items()} == meta["state_dict"] and len(spec) == 122
    assert sum(int(np.prod(v)) for v in spec.values()) == sum(int(np.prod(v)) for v in meta["state_dict"].values())
    sd = weights()
    assert sorted(sd) == sorted(spec) and all(sd[k].shape == tuple(spec[k]) and sd[k].dtype == np.float32 for k in spec)
    assert FD.FastDiffConfig.from_hparams({"fastdiff_upsample_ratios": (8, 8, 4), "fastdiff_T": 1000}) == FD.FastDiffConfig()


@pytest.mark.parametrize("N", [4, 3])
def test_inference_schedule_is_the_references_exactly(N):
    """inference_schedule runs the reference's float32 tensor operations in its order: the comparison is exact.  The C side
    (fs2_fd_schedule, what fs2_fd_sample uses) restates them in scalar float arithmetic: exact as well for the tabulated N = 3, 4."""
    fx = fixture("long")
    got = FD.inference_schedule(N)
    for k in ("beta", "alpha", "sigma", "steps"):
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].numpy(), fx[f"sched{N}_{k}"]), k
    want = {4: [7.4132, 23.4676, 74.9923, 498.0537], 3: [3.6308, 42.1119, 429.1123]}[N]
    assert np.allclose(got["steps"].numpy(), want, atol=5e-5, rtol=0)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    arrs = [(C.c_float * 8)() for _ in range(4)]
    assert lib.fs2_fd_schedule(N, *arrs) == _lib.FS2_OK
    for k, a in zip(("beta", "alpha", "sigma", "steps"), arrs):
        assert np.array_equal(np.asarray(a[:N], np.float32), fx[f"sched{N}_{k}"]), k
    assert lib.fs2_fd_schedule(5, *arrs) == _lib.FS2_ERR_SHAPE and lib.fs2_fd_schedule(200, *arrs) == _lib.FS2_ERR_SHAPE
    with pytest.raises(ValueError):
        FD.inference_schedule(5)


@pytest.mark.parametrize("case", CASES)
def test_float32_restatement_reproduces_the_reference(case):
    fx, ref = fixture(case), ref32()
    seen = {}
    for b, f in enumerate(fx["lengths"]):
        n = int(f) * 256
        mel = torch.as_tensor(fx["mel"][b, :f])
        for i in range(2):
            e = ref.eps(torch.as_tensor(fx["noise"][0, b, :n]), mel, float(fx["eps_steps"][i])).numpy()
            want = fx[f"eps_{i}"][b, :n]
            seen[f"eps_{i}"] = max(seen.get(f"eps_{i}", 0.0), float(np.abs(e - want).max()))
            if i == 0:
                assert 0.5 <= e.std() <= 2.0, (case, b, e.std())  # synth_state_dict's condition: eps is O(1)
        for N in (4, 3):
            w = ref.inference(mel, [torch.as_tensor(fx["noise"][j, b, :n]) for j in range(N)], schedule(fx, N)).numpy()
            seen[f"wav_n{N}"] = max(seen.get(f"wav_n{N}", 0.0), float(np.abs(w - fx[f"wav_n{N}"][b, :n]).max()))
            assert np.abs(w).max() == 1.0
    for k, got in seen.items():
        bound = MARGIN * float(fx[k + "_err64"])
        print(f"{case} {k}: restatement vs reference {got:.3e}, reference vs float64 {float(fx[k + '_err64']):.3e}")
        assert got <= bound, (case, k, got, bound)


def test_draw_noise_reproduces_the_seeded_run():
    """torch.manual_seed + draw_noise = the reference's own draws, utterance after utterance, x_T first"""
    fx, ref = fixture("ragged"), ref32()
    torch.manual_seed(fx["meta"]["run_seed"])
    noise = FD.draw_noise(fx["lengths"], 4)
    assert tuple(noise.shape) == (4, 3, 7 * 256) and float(noise[:, 2, 256:].abs().max()) == 0.0
    worst = 0.0
    for b, f in enumerate(fx["lengths"]):
        n = int(f) * 256
        w = ref.inference(torch.as_tensor(fx["mel"][b, :f]), [noise[j, b, :n] for j in range(4)], schedule(fx, 4)).numpy()
        worst = max(worst, float(np.abs(w - fx["wav_seeded"][b, :n]).max()))
    assert worst <= MARGIN * float(fx["wav_n4_err64"]), worst
    gen = torch.Generator().manual_seed(7)
    a = FD.draw_noise([2, 1], 3, generator=gen)
    torch.manual_seed(7)
    want = [torch.normal(0, 1, size=(1, 1, s)) for s in (512, 512, 512, 256, 256, 256)]
    assert torch.equal(a[:, 0, :], torch.stack([w.view(-1) for w in want[:3]])) and torch.equal(a[:, 1, :256], torch.stack([w.view(-1) for w in want[3:]]))


def test_bf16_hook_rounds_where_documented():
    """the storage hook changes the result by bf16-sized amounts only, and a value it returns is a bf16 value"""
    fx = fixture("ragged")
    mel, x = torch.as_tensor(fx["mel"][2, :1]), torch.as_tensor(fx["noise"][0, 2, :256])
    e64 = R.FastDiffRef(weights(), torch.float64).eps(x, mel, 74.99)
    e16 = R.FastDiffRef(weights(), torch.float64, R.bf16_round).eps(x, mel, 74.99)
    d = float((e64 - e16).abs().max())
    assert 1e-4 < d < 0.2, d
    t = torch.randn(64, dtype=torch.float64)
    assert torch.equal(R.bf16_round(t), R.bf16_round(R.bf16_round(t)))


def test_unsupported_configurations_are_refused_on_the_host():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert FD.FastDiffConfig().supported()
    for kw in ({"inner_channels": 64}, {"upsample_ratios": [8, 8, 2, 2]}, {"upsample_ratios": [4, 8, 8]}, {"lvc_layers_each_block": 3},
               {"kpnet_hidden_channels": 128}, {"cond_channels": 100}, {"diffusion_step_embed_dim_mid": 256}):
        cfg = FD.FastDiffConfig(**kw)
        assert not cfg.supported(), kw
        r = (C.c_int32 * len(cfg.upsample_ratios))(*cfg.upsample_ratios)
        h = C.c_void_p()
        assert lib.fs2_fd_create(_lib.FS2_ABI_VERSION, _lib.FS2_F32, *cfg._c_args(r), C.byref(h)) == _lib.FS2_ERR_SHAPE
        assert b"default architecture" in lib.fs2_fd_last_error(h)
        lib.fs2_fd_destroy(h)
    cfg = FD.FastDiffConfig()
    r = (C.c_int32 * 3)(8, 8, 4)
    h = C.c_void_p()
    assert lib.fs2_fd_create(_lib.FS2_ABI_VERSION, _lib.FS2_F16, *cfg._c_args(r), C.byref(h)) == _lib.FS2_ERR_ARG
    lib.fs2_fd_destroy(h)
    assert lib.fs2_fd_create(_lib.FS2_ABI_VERSION, _lib.FS2_F32, *cfg._c_args(r), C.byref(h)) == _lib.FS2_OK
    bad = np.zeros((32, 32, 5), np.float32)
    shp = (C.c_int64 * 3)(*bad.shape)
    assert lib.fs2_fd_load_weight(h, b"downsample.0.conv.0.weight", bad.ctypes.data_as(C.c_void_p), shp, 3) == _lib.FS2_ERR_WEIGHT
    assert b"shape mismatch" in lib.fs2_fd_last_error(h)
    assert lib.fs2_fd_load_weight(h, b"downsample.0.conv.9.weight", bad.ctypes.data_as(C.c_void_p), shp, 3) == _lib.FS2_ERR_WEIGHT
    assert lib.fs2_fd_launches(h, 0) == 71 and lib.fs2_fd_launches(h, 4) == 4 * 72 + 1
    assert lib.fs2_fd_hop(h) == 256 and lib.fs2_fd_tile_rows(h) == 64
    lib.fs2_fd_destroy(h)
    # the kernel order is a permutation of a frame's 24576 values, for both storage types
    for dt in (_lib.FS2_F32, _lib.FS2_BF16):
        idx = sorted(lib.fs2_fd_kernel_index(dt, l, c, o, k) for l in range(4) for c in range(32) for o in range(64) for k in range(3))
        assert idx == list(range(24576))
