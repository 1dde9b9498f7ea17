"""CPU restatement of the training attention (csrc/attention.hip, csrc/attention_pipe.hip forward with its by-products; csrc/backward.hip
attn_delta; csrc/attention_bwd.hip), in closed form - no autograd - and in three modes:

  f64   the truth: softmax(q k^T / sqrt(d) + key padding) -> dropout -> @ v and its gradients, float64 throughout
  f32   the same formulas in float32: the fp32 yardstick for lse2 and delta
  bf16  float64 with ONE round-to-nearest-even to bfloat16 exactly where the kernels round:

    forward (the training instantiations, TR / TRAIN: q enters the MFMA unscaled and the fp32 scores are scaled afterwards, so the
    scores are those of the backward; the inference instantiations round q log2(e)/sqrt(d) to bf16 instead and are not restated here)
      P (after dropout and its 1/(1-p)) -> bf16          attention.hip:354, 366 (pack_bounded of the dropped, rescaled exponentials),
                                                         attention_pipe.hip:286 (pack_bf16x2; this kernel runs without dropout only);
                                                         the row sum l adds the UNROUNDED, undropped fp32 exponentials
                                                         (attention.hip:336-341, attention_pipe.hip:284-285)
      out = (sum_k P v) / l -> bf16                      attention.hip:447-453, attention_pipe.hip:582-591
      lse2 = reference + log2(l), fp32                   attention.hip:438, attention_pipe.hip:572
    delta = sum_d dO out, fp32, from the bf16 out        backward.hip:439
    backward (both kernels recompute P = exp2((q . k) c - lse2): attention_bwd.hip:153, 282)
      pack4(pv): dropout(P) -> bf16                      attention_bwd.hip:165 (dK dV kernel; the dQ kernel needs no P operand)
      pack4(dsv): dS = P/sqrt(d) (dropout(dP) - delta)   attention_bwd.hip:166 (dK dV kernel), attention_bwd.hip:290 (dQ kernel)
      dK, dV, dQ -> bf16                                 attention_bwd.hip:199, 200, 310

Everything between those points is exact here and fp32 on the device (MFMA accumulation of exact bf16 products, v_exp_f32, v_log_f32).

Layouts as on the device: qkv (B*S, 3H) packed [q | k | v], head h in columns h*d .. h*d + d - 1 of each third; dout, out, dq, dk, dv
(B*S, H); pad (B, S) True at padded KEYS (padded queries are computed like any other); keep (B, heads, S, S) True where the weight
survives dropout; lse2, delta (B, heads, S).  lse2 is in log2 units of the scaled scores: sum_valid exp2(s c - lse2) = 1."""
import math

import torch

LOG2E = 1.4426950408889634


def bf16_round(x):
    """round-to-nearest-even to 8 significant bits, in x's own dtype (no detour through float32: no double rounding)"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def bf16_trunc(x):
    """the damaged store: chop to 8 significant bits"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.trunc(m * 256.0) / 256.0, e)


def heads_of(x, B, S, heads):
    """(B*S, heads*d) -> (B, heads, S, d)"""
    return x.view(B, S, heads, -1).transpose(1, 2)


def rows_of(x):
    """(B, heads, S, d) -> (B*S, heads*d)"""
    B, h, S, d = x.shape
    return x.transpose(1, 2).reshape(B * S, h * d)


def split_qkv(qkv, B, S, heads, dt):
    H = qkv.shape[1] // 3
    return tuple(heads_of(t.to(dt), B, S, heads) for t in qkv.view(B * S, 3 * H).split(H, dim=-1))


def scores2(qkv, pad, B, S, heads, dt=torch.float64):
    """(B, heads, S, S) scaled scores (q . k) log2(e)/sqrt(d) in log2 units, -inf at padded keys"""
    q, k, _ = split_qkv(qkv, B, S, heads, dt)
    s = (q @ k.transpose(-1, -2)) * torch.tensor(LOG2E / math.sqrt(q.shape[-1]), dtype=dt)
    return s.masked_fill(pad[:, None, None, :], float("-inf"))


def lse2_of(s2):
    m = s2.max(dim=-1, keepdim=True).values
    return (m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True)))[..., 0]


def delta_of(dout, out, B, S, heads, dt=torch.float64):
    """(B, heads, S): sum_d dO out of the tensors given (the device takes its own bf16 out)"""
    return (heads_of(dout.to(dt), B, S, heads) * heads_of(out.to(dt), B, S, heads)).sum(-1)


def attention_train(qkv, pad, dout, B, S, heads, keep=None, p=0.0, mode="f64", rnd=None, lse2=None, out=None, damage=None):
    """-> dict(out, lse2, delta, dq, dk, dv).  ``lse2`` / ``out``: take these (the device's) into delta and the backward in place of
    the restatement's own.  ``rnd``: the rounding of mode "bf16" (bf16_round; bf16_trunc for the damaged one).  ``damage``:
    {"dq_block": (b, h, k0)} drops keys k0 .. k0+15 from dQ of (b, h); {"lse_row": (b, h, q, shift)} shifts one row's lse2."""
    assert mode in ("f64", "f32", "bf16")
    dt = torch.float32 if mode == "f32" else torch.float64
    r = (rnd or bf16_round) if mode == "bf16" else (lambda x: x)
    damage = damage or {}
    q, k, v = split_qkv(qkv, B, S, heads, dt)
    d = q.shape[-1]
    scale = torch.tensor(1.0 / math.sqrt(d), dtype=dt)
    c = torch.tensor(LOG2E / math.sqrt(d), dtype=dt)
    dsc = 1.0 / (1.0 - p) if p > 0 else 1.0
    km = torch.ones(B, heads, S, S, dtype=dt) if keep is None else keep.to(dt)
    padk = pad[:, None, None, :]
    # ---- forward
    s2f = ((q @ k.transpose(-1, -2)) * c).masked_fill(padk, float("-inf"))
    m = s2f.max(dim=-1, keepdim=True).values
    e = torch.exp2(s2f - m)
    l = e.sum(-1, keepdim=True)
    own_lse = (m + torch.log2(l))[..., 0]
    own_out = r(rows_of((r(e * km * dsc) @ v) / l))
    if "lse_row" in damage:
        b_, h_, q_, sh = damage["lse_row"]
        own_lse = own_lse.clone()
        own_lse[b_, h_, q_] += sh
    lse = own_lse if lse2 is None else lse2.to(dt)
    o = own_out if out is None else out.to(dt)
    # ---- backward: P from the same scores and the forward's lse2
    do = heads_of(dout.to(dt), B, S, heads)
    delta = delta_of(dout, o, B, S, heads, dt)
    P = torch.exp2(s2f - lse[..., None])
    dP = do @ v.transpose(-1, -2)
    pd = r(P * km * dsc)
    dS = r((P * scale) * (dP * km * dsc - delta[..., None]))
    dSq = dS
    if "dq_block" in damage:
        b_, h_, k0 = damage["dq_block"]
        dSq = dS.clone()
        dSq[b_, h_, :, k0:k0 + 16] = 0
    return {"out": own_out, "lse2": own_lse, "delta": delta,
            "dq": r(rows_of(dSq @ k)), "dk": r(rows_of(dS.transpose(-1, -2) @ q)), "dv": r(rows_of(pd.transpose(-1, -2) @ do))}


def autograd_truth(qkv, pad, dout, B, S, heads, keep=None, p=0.0):
    """float64 autograd of softmax(q k^T / sqrt(d) + key padding) -> dropout -> @ v: what the closed form must equal"""
    q, k, v = (t.clone().requires_grad_(True) for t in split_qkv(qkv, B, S, heads, torch.float64))
    d = q.shape[-1]
    s = (q @ k.transpose(-1, -2) / math.sqrt(d)).masked_fill(pad[:, None, None, :], float("-inf"))
    P = torch.softmax(s, dim=-1)
    if keep is not None:
        P = P * keep.double() / (1.0 - p)
    out = rows_of(P @ v)
    out.backward(dout.double())
    return {"out": out.detach(), "lse2": torch.logsumexp(s.detach(), dim=-1) * LOG2E,
            "dq": rows_of(q.grad), "dk": rows_of(k.grad), "dv": rows_of(v.grad)}


# ---- the judges (tests/test_gpu_fastdiff_edges.py's convention) ----
EPS32 = 2.0 ** -23
MARGIN = 4


def errs(a, truth):
    dlt = (a.double() - truth.double()).reshape(-1)
    if dlt.numel() == 0:
        return 0.0, 0.0
    return float(dlt.abs().max()), float(dlt.pow(2).mean().sqrt())


def fp32_bound(y32, truth):
    """MARGIN x max(float32 restatement's max error, 2^-23 max|truth|)"""
    return MARGIN * max(errs(y32, truth)[0], EPS32 * float(truth.abs().max()))


def grad_floor(qkv, dout, B, S, heads):
    """What fp32 accumulation alone may leave in a gradient element, from the formats: dP and delta are two fp32 sums of d products
    bounded by A = max_(q,k) sum_i |dO_qi| |v_ki|, formed in different orders, so (dP - delta) carries up to 2^-23 A; times
    P / sqrt(d) <= 1 / sqrt(d) and one operand element <= max|qkv| (the probabilities of a row sum to 1).  It matters only where the
    bf16 restatement's own error is zero (utterances of ONE key: P = 1, dP = delta, dS = 0 exactly); elsewhere it is below 2 % of
    the 2 x bound (tests/test_attn_train_ref_cpu.py asserts that)."""
    _, _, v = split_qkv(qkv, B, S, heads, torch.float64)
    A = float((heads_of(dout.double(), B, S, heads).abs() @ v.abs().transpose(-1, -2)).max())
    return MARGIN * EPS32 * A * float(qkv.abs().max()) / math.sqrt(v.shape[-1])


def ratio_2x(got, truth, model, floor=0.0):
    """-> (passes, figures): the bf16 rule, max-abs and rms of (got - truth) at most 2 x the restatement's (+ the fp32 floor)"""
    eg, ey = errs(got, truth), errs(model, truth)
    ok = eg[0] <= 2 * ey[0] + floor and eg[1] <= 2 * ey[1] + floor
    return ok, {"dev_max": eg[0], "dev_rms": eg[1], "ref_max": ey[0], "ref_rms": ey[1],
                "ratio_max": eg[0] / ey[0] if ey[0] else float("nan"), "ratio_rms": eg[1] / ey[1] if ey[1] else float("nan")}


# ---- inputs shared by the CPU and the GPU file ----
def mask_of(kind, B, S):
    """the mask shapes of tests/test_gpu_ops._mask"""
    mask = torch.zeros(B, S, dtype=torch.bool)
    if kind == "suffix":
        for b in range(B):
            mask[b, S - (7 + 13 * b) % S:] = True
        mask[0, :] = False
        mask[0, S - S // 2:] = True
    elif kind == "scatter":
        mask = torch.rand(B, S, generator=torch.Generator().manual_seed(11)) < 0.3
        mask[:, 0] = False
    elif kind == "prefix":
        mask[:, :S - min(S, 40)] = True
    elif kind == "holes":
        mask[:, 64:192] = True
        mask[1 % B, 200:S - 3] = True
    return mask


def inputs(B, S, heads, seed, d=128):
    """qkv (B*S, 3H) = 0.5 randn and dout (B*S, H) = randn, both bf16 VALUES held in float32: exact for every judge"""
    g = torch.Generator().manual_seed(seed)
    H = heads * d
    qkv = (0.5 * torch.randn(B * S, 3 * H, generator=g)).to(torch.bfloat16).float()
    dout = torch.randn(B * S, H, generator=g).to(torch.bfloat16).float()
    return qkv, dout


FORWARD_CASES = [(2, 200, 2, "suffix"), (3, 130, 1, "suffix"), (2, 257, 2, "scatter"), (2, 300, 2, "prefix"), (2, 450, 2, "holes"),
                 (1, 1, 1, "none")]
# by size: the smallest shapes with heads * ceil(S / 128) >= 16, and one unit below each
BYSIZE_CASES = [((2, 70, 16), (2, 70, 15)), ((1, 129, 16), (1, 129, 7)), ((2, 385, 6), (2, 385, 3)), ((1, 897, 2), (1, 897, 1))]
SEAM_S = [1, 17, 63, 64, 65, 129, 193, 257]


def seam_lengths(S):
    return (S, 1, max(1, S - 70))


def far_rows_qkv():
    """tests/test_gpu_ops.py test_attention_pipelined_rows_far_below_and_above_zero: S = 512, one head; every key carries a large
    component along -q7 (query 7: all scores ~ -160 log2 units) and along +q9 (~ +160); the last 50 keys padded"""
    B, S, H = 1, 512, 128
    qkv = torch.randn(B * S, 3 * H, generator=torch.Generator().manual_seed(31))
    q = qkv[:, :H].clone()
    qkv[:, H:2 * H] *= 0.3
    d7, d9 = q[7] / q[7].norm(), q[9] / q[9].norm()
    qkv[:, H:2 * H] += (-1250.0 / float(q[7].norm())) * d7 + (1250.0 / float(q[9].norm())) * d9
    pad = torch.zeros(B, S, dtype=torch.bool)
    pad[0, S - 50:] = True
    return qkv.to(torch.bfloat16).float(), pad, (B, S, 1), (7, 9)


def spike_qkv():
    """test_attention_pipelined_spike_and_all_padded: S = 512, B = 2, two heads; key 300 = 8 x query 5 (utterance 0, head 0), key 450 =
    -9 x query 77 (utterance 1, head 1)"""
    B, S, H = 2, 512, 256
    qkv = torch.randn(B * S, 3 * H, generator=torch.Generator().manual_seed(12))
    qkv[300, H:H + 128] = 8.0 * qkv[5, :128]
    qkv[S + 450, H + 128:H + 256] = -9.0 * qkv[S + 77, 128:256]
    return qkv.to(torch.bfloat16).float(), torch.zeros(B, S, dtype=torch.bool), (B, S, 2), (5, S + 77)
