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


def c_schedule(N):
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    arrs = [(C.c_float * 8)() for _ in range(4)]
    assert _lib.load().fs2_fd_schedule(N, *arrs) == _lib.FS2_OK
    return {k: np.asarray(a[:N], np.float32) for k, a in zip(("beta", "alpha", "sigma", "steps"), arrs)}


def ulps(a, b):
    """a - b in units in the last place, for float32 arrays of one sign"""
    return (a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).tolist()


def test_schedule_n8_is_the_references_exactly():
    """N = 8: inference_schedule, the reference's record and the C side agree bit for bit"""
    fx, want, got = fixture("ragged_n68"), FD.inference_schedule(8), c_schedule(8)
    for k in ("beta", "alpha", "sigma", "steps"):
        assert want[k].dtype == torch.float32 and np.array_equal(want[k].numpy(), fx[f"sched8_{k}"]), k
        assert np.array_equal(got[k], want[k].numpy()), (k, ulps(got[k], want[k].numpy()))
    assert (np.diff(got["steps"]) > 0).all() and 0 <= got["steps"][0] and got["steps"][-1] < 999


def test_schedule_n6_departs_from_the_reference_where_documented_and_nowhere_else():
    """N = 6, the one documented departure (inference_schedule's docstring): the cumulative alpha of step 4, 0.94868..., is the
    square root of a near-tie.  The C side's sqrtf is correctly rounded; the torch.sqrt of the reference's recorded run rounded this
    one the other way.  So the C side's alpha[4] lies exactly ONE ulp above the reference's, and its fractional step 144.46 exactly
    SIX ulps (9.2e-5) below.  Every other entry of the four arrays is the reference's, bit for bit.  (What this does to the
    waveform: tests/test_gpu_fastdiff_edges.py::test_inference_n6_fp32 measures it)

    The reference's side is its RECORD (sched6_* of the fixture, written by the unmodified reference): what torch.sqrt returns live
    differs from CPU to CPU by more than this (on one host at a fifth of all inputs), so inference_schedule takes its three square
    roots correctly rounded and equals the C side bit for bit, here as for every N (asserted below and in the tests above)."""
    fx, mirror, got = fixture("ragged_n68"), FD.inference_schedule(6), c_schedule(6)
    for k in ("beta", "alpha", "sigma", "steps"):
        assert mirror[k].dtype == torch.float32 and np.array_equal(got[k], mirror[k].numpy()), (k, ulps(got[k], mirror[k].numpy()))
        d = ulps(got[k], fx[f"sched6_{k}"])
        print(f"N = 6 {k}: C side - the reference's record in ulps {d}")
        assert d == {"alpha": [0, 0, 0, 0, 1, 0], "steps": [0, 0, 0, 0, -6, 0]}.get(k, [0] * 6), (k, d)
    # the C side is the correctly rounded one: a float64 square root rounded to float32 is the correctly rounded float32 square
    # root (53 >= 2 x 24 + 2 significand bits)
    a = np.float32(1) - np.asarray(FD._BETAS[6], np.float32)
    prod = np.multiply.accumulate(a, dtype=np.float32)
    assert np.array_equal(np.sqrt(prod.astype(np.float64)).astype(np.float32), got["alpha"])
    assert abs(float(got["steps"][4]) - 144.4617) < 1e-3 and abs(float(got["steps"][4]) - float(fx["sched6_steps"][4]) + 9.2e-5) < 1e-5


def test_inference_schedule_takes_its_square_roots_correctly_rounded():
    """the hook: sqrt=torch.sqrt is the reference's own operation (host dependent, what the fixture tool records); the default is
    the correctly rounded root of every element, whatever this host's torch.sqrt makes of it"""
    t = torch.linspace(0.25, 1.0, 4097)
    want = np.sqrt(t.numpy().astype(np.float64)).astype(np.float32)
    assert np.array_equal(FD._sqrt_rounded(t).numpy(), want) and FD._sqrt_rounded(t).dtype == torch.float32
    seen = []
    FD.inference_schedule(3, sqrt=lambda v: seen.append(v.numel()) or torch.sqrt(v))
    assert seen == [1000, 3, 3]


@pytest.mark.parametrize("hop,lengths,T", [(8, (7, 4, 1), 7), (64, (7, 4, 1), 7), (256, (7, 4, 1), 7), (8, (9, 3), 9)])
def test_bf16_elementwise_bound_holds_for_the_rounded_float32_restatement(hop, lengths, T):
    """The rule tests/test_gpu_fastdiff_edges.py::test_op_lvc_bf16 holds the device to, checked on its own model first: the float32
    restatement of the launch on bf16-exact inputs, rounded ONCE to bf16 (round to nearest), meets it at every element, layer and
    hop; the same values TRUNCATED to bf16 (an error of up to 2^-7 |truth|) do not."""
    inp = R.lvc_op_inputs(hop, lengths, T, seed=hop + T, bf16=True)
    for layer in range(4):
        for b, f in enumerate(lengths):
            t64 = R.lvc_op_ref(inp, b, f, hop, layer, torch.float64)
            t32 = R.lvc_op_ref(inp, b, f, hop, layer, torch.float32)
            for truth, r32 in zip(t64, t32):
                truth = truth.numpy()
                yard = float(np.abs(r32.double().numpy() - truth).max())
                assert R.bf16_elementwise_excess(R.bf16_round(r32).numpy(), truth, yard, MARGIN) <= 0, (hop, layer, b)
                cut = (r32.contiguous().view(torch.int32) & -65536).view(torch.float32).numpy()
                assert R.bf16_elementwise_excess(cut, truth, yard, MARGIN) > 0, (hop, layer, b)


@pytest.mark.parametrize("case", CASES + ("ragged_n68",))
def test_float32_restatement_reproduces_the_reference(case):
    fx, ref = fixture(case), ref32()
    seen = {}
    for b, f in enumerate(fx["lengths"]):
        n = int(f) * 256
        mel = torch.as_tensor(fx["mel"][b, :f])
        for i in range(2 if "eps_0" in fx else 0):
            e = ref.eps(torch.as_tensor(fx["noise"][0, b, :n]), mel, float(fx["eps_steps"][i])).numpy()
            want = fx[f"eps_{i}"][b, :n]
            seen[f"eps_{i}"] = max(seen.get(f"eps_{i}", 0.0), float(np.abs(e - want).max()))
            if i == 0:
                assert 0.5 <= e.std() <= 2.0, (case, b, e.std())  # synth_state_dict's condition: eps is O(1)
        for N in [N for N in (4, 3, 6, 8) if f"wav_n{N}" in fx]:  # ragged, long: 4 and 3; ragged_n68: 6 and 8
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


@pytest.mark.parametrize("dtype", [_lib.FS2_F32, _lib.FS2_BF16])
def test_workspace_bytes_follow_the_headers_rule(dtype):
    """fs2_fd_workspace_bytes is host arithmetic (no launch, no device).  The rule of include/fs2.h, read from the code: the workspace
    is the layout of ONE chunk, and a chunk holds min(B, limit) utterances, where the limit is fs2_fd_set_chunk's or, by default,
    fit = max(1, floor(2 GiB / bytes(1, T))): as many as fit 2 GiB, at least one.  So bytes(B, T) = layout(min(B, fit), T), and
    layout(n, T) itself can be read as bytes(n, T) under set_chunk(n)."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib, cfg = _lib.load(), FD.FastDiffConfig()
    h = C.c_void_p()
    assert lib.fs2_fd_create(_lib.FS2_ABI_VERSION, dtype, *cfg._c_args((C.c_int32 * 3)(8, 8, 4)), C.byref(h)) == _lib.FS2_OK

    def ws(B, T, limit=0):
        n = C.c_size_t()
        assert lib.fs2_fd_set_chunk(h, limit) == _lib.FS2_OK and lib.fs2_fd_workspace_bytes(h, B, T, C.byref(n)) == _lib.FS2_OK
        assert lib.fs2_fd_set_chunk(h, 0) == _lib.FS2_OK
        return n.value
    try:
        cap, T = 2 << 30, 1536
        sizes = [ws(B, T) for B in range(1, 41)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] % 256 == 0  # non-decreasing in B
        fit = max(1, cap // sizes[0])
        assert fit == {_lib.FS2_F32: 5, _lib.FS2_BF16: 11}[dtype]  # profiles/fastdiff.md: utterances per chunk at 32 x 1536
        assert ws(32, T) == ws(fit, T) == ws(fit, T, limit=fit) <= cap  # the flagship batch: exactly layout(fit, T), under the cap
        assert ws(fit + 1, T, limit=fit + 1) > cap                        # ... and one utterance more would not have fitted
        assert all(s == ws(B, T, limit=B) for B, s in enumerate(sizes[:fit], 1))  # B <= fit: the whole batch in one chunk
        assert len(set(sizes[fit - 1:])) == 1
        # one utterance larger than the cap: still a size, that of one utterance ("at least one"), whatever B
        big = ws(1, 32768)
        assert big > cap and ws(8, 32768) == big == ws(8, 32768, limit=1)
        # a limit of one utterance: B does not matter
        assert ws(1, T, limit=1) == ws(8, T, limit=1) == sizes[0] and ws(1, 7, limit=1) == ws(8, 7, limit=1) < ws(8, 7)
        assert lib.fs2_fd_set_chunk(h, -1) == _lib.FS2_ERR_ARG and lib.fs2_fd_workspace_bytes(h, 0, T, C.byref(C.c_size_t())) == _lib.FS2_ERR_ARG
    finally:
        lib.fs2_fd_destroy(h)
