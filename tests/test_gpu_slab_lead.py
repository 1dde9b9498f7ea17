"""The slab GEMM's lead-2 K loop (gemm_mfma.hip: three weight stages, the tile of step s + 2 requested at the top of step s, a
counted wait) against its two-stage loop, through the operator entry points: knob 240 = two stages everywhere, 242 = the lead-2
loop wherever it exists.  Same MFMA sequence per output element, so every comparison is torch.equal on the stored bits.
Knobs 6 / 7 / 3 / 4 force 32- / 64- / 128- / 192-row tiles; two utterances of a ragged length, so that tiles end inside an
utterance's last rows (conv launches) or run across its end (pointwise launches) and the last tile has a row tail."""
import pytest
import torch

import _gpu as G

pytestmark = pytest.mark.gpu

HEIGHT_KNOB = {32: 6, 64: 7, 128: 3, 192: 4}
B, S = 2, 200  # 400 rows: 128-row tiles 0-127, 128-255 (across the utterance end), 256-383, 384-399; per utterance 128 + 72


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


BIAS, RES, LN, LNTMP, STATS, EPIRES, RELU = 1 << 0, 1 << 1, 1 << 2, 1 << 5, 1 << 6, 1 << 7, 1 << 16  # fs2_op_gemm_route's `present` bits


def both(rows, run, req, form):
    """run() under the two-stage loop and under the lead-2 loop, at the forced tile height.  req = (dtype, M, N, Cin, taps, S, present):
    the launcher's own answer (fs2_op_gemm_route_lead) must be `form` under 242 - 1 pointwise, 2 conv, 0 where the loop does not exist
    (the comparison is then two-stage against two-stage and says nothing) - and 0 under 240, so a dead dispatch cannot pass."""
    lib = G.lib()
    dt, M, N, Cin, taps, s, present = req
    lead = lambda: lib.fs2_op_gemm_route_lead(dt, dt, M, N, Cin, taps, s, 0, present, 1)
    try:
        assert lib.fs2_op_set_gemm_variant(HEIGHT_KNOB[rows]) == 0
        assert lib.fs2_op_set_gemm_variant(240) == 0
        assert lead() == 0
        old = run()
        assert lib.fs2_op_set_gemm_variant(242) == 0
        assert lead() == form, (lead(), form)
        new = run()
    finally:
        lib.fs2_op_set_gemm_variant(241)
        lib.fs2_op_set_gemm_variant(0)
    return old, new


def same(old, new, what):
    old = old if isinstance(old, (tuple, list)) else (old,)
    new = new if isinstance(new, (tuple, list)) else (new,)
    for i, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), (what, i)


def test_knob_pair_is_defined():
    lib = G.lib()
    try:
        for v in (240, 242, 241):
            assert lib.fs2_op_set_gemm_variant(v) == 0
        assert lib.fs2_op_set_gemm_variant(243) != 0 and lib.fs2_op_set_gemm_variant(211) != 0
    finally:
        lib.fs2_op_set_gemm_variant(241)


@pytest.mark.parametrize("rows", [32, 64, 128, 192])
@pytest.mark.parametrize("K", [64, 128, 192, 256])
def test_pointwise_step_counts_around_the_ring_depth(rows, K):
    """1, 2, 3 and 4 K steps: the prologue has two tiles in flight, the ring has three stages - where a counted wait goes wrong"""
    x, w, b = rnd(B * S, K, seed=1), rnd(256, K, seed=2, scale=K ** -0.5), rnd(256, seed=3)
    old, new = both(rows, lambda: G.gemm(G.BF16, x, w, b, raw=True), (G.BF16, B * S, 256, K, 1, B * S, BIAS), 1)
    same(old, new, (rows, K))
    ref = G.rounded(x, G.BF16) @ G.rounded(w, G.BF16).T + b
    assert float((new.float() - ref).abs().max()) <= 1.2e-2 * float(ref.abs().max())


@pytest.mark.parametrize("rows", [32, 64, 128])
@pytest.mark.parametrize("k,Cin", [(3, 64), (9, 128), (9, 256)])
def test_conv_forms(rows, k, Cin):
    """k = 3 with one channel block (3 steps); k = 9 with two and four (the next block's slab requested mid-loop, behind a weight
    tile); one column tile and a column tail (N = 320); with and without ReLU"""
    x = rnd(B * S, Cin, seed=4)
    for N in (256, 320):
        w, b = rnd(N, k * Cin, seed=5 + N, scale=(k * Cin) ** -0.5), rnd(N, seed=6)
        for relu in (False, True):
            old, new = both(rows, lambda: G.gemm(G.BF16, x, w, b, taps=k, S=S, relu=relu, raw=True),
                            (G.BF16, B * S, N, Cin, k, S, BIAS | (RELU if relu else 0)), 2)
            same(old, new, (rows, k, Cin, N, relu))


@pytest.mark.parametrize("rows", [128, 192])
@pytest.mark.parametrize("K,k,relu,res", [(256, 1, False, True), (1024, 1, False, True), (256, 3, True, False)])
def test_layernorm_epilogue(rows, K, k, relu, res):
    """the fused LayerNorm epilogue behind the lead-2 loop: the residual in the accumulators (its loads go out behind the first
    requests), the ReLU form, the predictor head; y and the head prediction.  At 192 rows the loop does not exist with this epilogue
    (it spills there: not built) nor as a conv form (LDS): those cases pin that knob 242 changes nothing."""
    x = rnd(B * S, K, seed=7)
    w, b = rnd(256, k * K, seed=8, scale=(k * K) ** -0.5), rnd(256, seed=9)
    g, be, hw = rnd(256, seed=10), rnd(256, seed=11), rnd(256, seed=12)
    r = rnd(B * S, 256, seed=13) if res else None
    form = 0 if rows == 192 else 1 if k == 1 else 2
    req = (G.BF16, B * S, 256, K, k, S if k > 1 else B * S, BIAS | LN | LNTMP | (RES if res else 0) | (RELU if relu else 0) | 1 << 3)
    old, new = both(rows, lambda: G.gemm_ln(G.BF16, x, w, b, r, g, be, taps=k, S=S, relu=relu, dot_w=hw, dot_b=0.3, raw=True), req, form)
    same(old, new, (rows, K, k))
    assert torch.isfinite(new[0].float()).all() and torch.isfinite(new[1]).all()


@pytest.mark.parametrize("rows", [128, 192])
def test_deferred_layernorm_epilogue(rows):
    """N = 768, K = 256 with a residual: three column tiles, pre-norm rows and the row statistics (192 rows: no lead-2 form, as above)"""
    x, w, b = rnd(B * S, 256, seed=14), rnd(768, 256, seed=15, scale=1 / 16), rnd(768, seed=16)
    r = rnd(B * S, 768, seed=17)

    def run():
        v, st = G.gemm_stats(G.BF16, x, w, b, r)
        return v.cpu(), st.cpu()
    old, new = both(rows, run, (G.BF16, B * S, 768, 256, 1, B * S, BIAS | STATS | EPIRES), 1 if rows == 128 else 0)
    same(old, new, rows)
    assert torch.isfinite(new[1]).all()


@pytest.mark.parametrize("k,Cin", [(1, 256), (9, 128)])
def test_f16(k, Cin):
    x, w, b = rnd(B * S, Cin, seed=18), rnd(320, k * Cin, seed=19, scale=(k * Cin) ** -0.5), rnd(320, seed=20)
    old, new = both(128, lambda: G.gemm(G.F16, x, w, b, taps=k, S=S, relu=True, raw=True),
                    (G.F16, B * S, 320, Cin, k, S if k > 1 else B * S, BIAS | RELU), 1 if k == 1 else 2)
    same(old, new, (k, Cin))
    assert new.dtype == torch.float16 and torch.isfinite(new.float()).all()


@pytest.mark.parametrize("k,Cin", [(1, 256), (9, 128), (3, 64)])
def test_tile_mostly_out_of_range(k, Cin):
    """S = 40 at 128-row tiles: 88 dead rows per tile, which read as zeros and are never stored"""
    s = 40
    x, w, b = rnd(B * s, Cin, seed=21), rnd(256, k * Cin, seed=22, scale=(k * Cin) ** -0.5), rnd(256, seed=23)
    old, new = both(128, lambda: G.gemm(G.BF16, x, w, b, taps=k, S=s, raw=True),
                    (G.BF16, B * s, 256, Cin, k, s if k > 1 else B * s, BIAS), 1 if k == 1 else 2)
    same(old, new, (k, Cin))
    xr, wr = G.rounded(x, G.BF16).reshape(B, s, Cin), G.rounded(w, G.BF16).reshape(256, k, Cin)
    xp = torch.nn.functional.pad(xr, (0, 0, k // 2, k // 2))
    ref = sum(xp[:, t:t + s] @ wr[:, t].T for t in range(k)).reshape(B * s, 256) + b
    assert float((new.float() - ref).abs().max()) <= 1.2e-2 * float(ref.abs().max())


@pytest.mark.parametrize("k,Cin", [(1, 256), (9, 128)])
def test_two_launches_back_to_back(k, Cin):
    """two launches into the same output with different inputs, nothing between them: the second one's bits are what it gives
    alone under the two-stage loop - nothing of the first is left pending"""
    lib = G.lib()
    M, N = B * S, 256
    x1, x2 = G.to_dev(rnd(M, Cin, seed=24), G.BF16), G.to_dev(rnd(M, Cin, seed=25), G.BF16)
    w1 = G.to_dev(rnd(N, k * Cin, seed=26, scale=(k * Cin) ** -0.5), G.BF16)
    w2 = G.to_dev(rnd(N, k * Cin, seed=27, scale=(k * Cin) ** -0.5), G.BF16)
    bd = rnd(N, seed=28).to(G.DEV)

    def run(pair):
        c = torch.zeros(M, N, dtype=torch.bfloat16, device=G.DEV)
        st = torch.cuda.current_stream()
        if pair:
            G.ok(lib.fs2_op_gemm(G.BF16, G.BF16, x1, w1, bd, c, M, N, Cin, k, S, 0, st), "gemm")
        G.ok(lib.fs2_op_gemm(G.BF16, G.BF16, x2, w2, bd, c, M, N, Cin, k, S, 0, st), "gemm")
        torch.cuda.synchronize()
        return c.cpu()
    try:
        assert lib.fs2_op_set_gemm_variant(HEIGHT_KNOB[128]) == 0 and lib.fs2_op_set_gemm_variant(240) == 0
        alone = run(False)
        assert lib.fs2_op_set_gemm_variant(242) == 0
        assert lib.fs2_op_gemm_route_lead(G.BF16, G.BF16, M, N, Cin, k, S, 0, BIAS, 1) == (1 if k == 1 else 2)
        pair, again = run(True), run(True)
    finally:
        lib.fs2_op_set_gemm_variant(241)
        lib.fs2_op_set_gemm_variant(0)
    assert torch.equal(pair, alone) and torch.equal(again, alone)
