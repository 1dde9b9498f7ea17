"""Host mirror of the reference's training step:

    FastSpeech2.training_step (litfass/fastspeech2/fastspeech2.py:786-797):  result = self(batch); losses = self.loss(result, batch)
    -> loss.backward() (Lightning) -> clip_grad_norm_(gradient_clip_val, scripts/train.sh:16)
    -> torch.optim.AdamW(lr, betas=[0.9, 0.98], eps=1e-8, weight_decay=0.01) + NoamLR (fastspeech2.py:1166-1182, noam.py:4-25)

built on the HIP operators behind the C ABI (include/fs2.h, "Training step" section): the teacher-forced forward keeps
every tensor the backward needs in HBM (288 GB: nothing is recomputed except the attention probabilities where the fused
attention + recomputing backward applies - bf16, head dim 128; elsewhere they are materialised),
the backward is a hand-written tape over fs2_op_bgemm / fs2_op_layernorm_bwd / fs2_op_attention_bwd / ..., parameters,
gradients and both Adam moments live in ONE flat fp32 buffer each so the optimizer is a single launch and a data-parallel
job all-reduces one contiguous gradient buffer.  torch supplies device memory and streams only; there is no autograd and
no CPU path - without libfs2_hip.so the constructor raises.

Covered: dense and depth-wise convolution variants of every block (C1-C5 of BASELINE.json, the reference's class defaults
and the test-size configs; the depth-wise layer's conv2 pair is trained through its folded (H, F) map), frame-level
'none' and phone-level / CWT variances, 'l1' / 'mse' losses; precision "fp32" (exact fp32 MFMA, the parity mode) or "bf16" (bf16 activations,
activation gradients and GEMM operands on the bf16 MFMA with fp32 accumulation; fp32 master weights, weight gradients,
Adam moments, LayerNorm / softmax statistics and losses - what the reference's `--precision 16` recipe does with fp16).
Dropout: every nn.Dropout site of the reference in training mode (encoder / decoder incl. the attention weights and both positional encodings, variance / duration predictors)
with a counter-based mask that is regenerated, not stored; 0 by default, which is what the parity fixtures pin (the
reference's masks come from torch's random stream and cannot be reproduced).  Priors (PriorEmbedding) are trained.  Variances at either level
("frame" / "phone") with either transform ("none" / "cwt": the 10-scale spectrogram head + the utterance-level mean / std head,
teacher-forced with the raw signal).  Rejected loudly: soft-DTW on a CWT spectrogram, stochastic durations.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .config import Fs2Config
from .weights import state_dict_spec

F32, BF16 = _lib.FS2_F32, _lib.FS2_BF16
_KIND = {"l1": 0, "mse": 1}
_PRECISIONS = {"fp32": (F32, torch.float32), "bf16": (BF16, torch.bfloat16)}


def _desc(c_dtype, **kw):
    """the descriptor of a strided-batched product: one plain product into c_dtype unless the fields say otherwise"""
    return _lib.BGemmDescC(**{"nb1": 1, "nb2": 1, "alpha": 1.0, "beta": 0.0, "splitk": 1, "taps": 1, "c_dtype": c_dtype, **kw})


class _Ops:
    """Thin typed wrappers: torch tensors in, C ABI launches on torch's current stream."""

    def __init__(self, device, precision="fp32"):
        self.lib = _lib.load()
        self.dt, self.tdt = _PRECISIONS[precision]   # activation dtype (C ABI enum, torch dtype)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("the training step runs on the GPU (no CPU path)")
        self._ws: Dict[str, torch.Tensor] = {}
        self.seed = 0       # dropout: set per micro-step by the trainer
        self._site = 0      # dropout site counter of the current forward
        self.fuse_ln = os.environ.get("FS2_TRAIN_FUSE_LN", "1") != "0"  # A/B switch: GEMM + LayerNorm as one launch where it applies
        self.fuse_ln_drop = os.environ.get("FS2_TRAIN_FUSE_LN_DROPOUT", "1") != "0"  # A/B switch: the residual-site dropout inside that launch
        self.fuse_add = os.environ.get("FS2_TRAIN_FUSE_ADD", "1") != "0"  # A/B switch: "dx +=" of a data-gradient product inside the GEMM launch
        self.splitk = os.environ.get("FS2_TRAIN_SPLITK", "1") != "0"    # A/B switch: split-K data-gradient convs where fs2_op_gemm_splitk_choice says so
        self.gate = os.environ.get("FS2_TRAIN_GATE", "1") != "0"        # A/B switch: the FFN's ReLU + dropout backward inside the data-gradient GEMM's store
        # Weight gradients are leaves of the backward: nothing downstream reads them before the optimizer step.  With
        # FS2_TRAIN_WGRAD_STREAM=1 they run on a second HIP stream (dW GEMM + split-K reduce + bias column sums: ~110 of a step's
        # ~510 launches) beside the data-gradient chain, ordered by events: the side stream waits for dy, the main stream waits
        # for the side stream before it overwrites a tensor a pending product still reads (_guard) and at the end of the step.
        # Measured r04 at C2, bf16: 10.95 -> 10.5 ms per step (12.30 -> 11.7 with the recipe's dropout); fp32 (long MFMA-bound launches,
        # nothing to fill) 63.2 -> 64.3, so the default follows the precision.  FS2_TRAIN_WGRAD_STREAM=0 / 1 overrides.
        side_on = os.environ.get("FS2_TRAIN_WGRAD_STREAM", "1" if precision == "bf16" else "0") == "1"
        self.side = torch.cuda.Stream(self.dev) if side_on else None
        self._ws_tag = ""
        self._pending: Dict[int, "torch.cuda.Event"] = {}

    def site(self):
        self._site += 1
        return self._site

    def st(self):
        return torch.cuda.current_stream(self.dev)

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.dev)

    def act(self, *shape):
        return torch.empty(*shape, dtype=self.tdt, device=self.dev)

    def to_act(self, x):
        """fp32 -> activation dtype (loss gradients enter the backward chain through this)"""
        if self.dt == F32:
            return x
        y = self.act(*x.shape)
        _lib.check(self.lib.fs2_op_convert(F32, self.dt, x, y, x.numel(), self.st()), None, "convert")
        return y

    @staticmethod
    def _base(t):
        return t.untyped_storage().data_ptr()

    def _guard(self, *tensors):
        """about to WRITE these tensors on the current stream: wait for side-stream products that still read them"""
        if not self._pending:
            return
        for t in tensors:
            ev = self._pending.pop(self._base(t), None) if t is not None else None
            if ev is not None:
                torch.cuda.current_stream(self.dev).wait_event(ev)

    def join_side(self):
        """the current stream waits for everything queued on the weight-gradient stream"""
        if self.side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self.side)
            self._pending.clear()

    @staticmethod
    def took(status, what):
        """the answer of a fused entry point: True = launched; False = FS2_ERR_SHAPE, "no such kernel for this shape" - the one status
        the caller answers with its stand-alone launches; anything else is a failure and raises"""
        if status == _lib.FS2_ERR_SHAPE:
            return False
        _lib.check(status, None, what)
        return True

    def ws(self, key: str, nbytes: int) -> Optional[torch.Tensor]:
        if nbytes <= 0:
            return None
        key = key + self._ws_tag  # the side stream's launches have workspaces of their own
        t = self._ws.get(key)
        if t is None or t.numel() * 4 < nbytes:
            # zeroed: the column-sum workspace starts with ticket counters that every launch returns to zero (include/fs2.h)
            t = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.dev)
            self._ws[key] = t
        return t

    # ---- forward operators (the inference path's own launches, fp32) ----
    def gemm(self, x, w, bias, M, N, Cin, taps=1, S=None, relu=False, out_f32=False, gate=None, gate_scale=1.0):
        y = self.empty(M, N) if out_f32 else self.act(M, N)
        if gate is not None:  # y = gate > 0 ? gate_scale * x w^T : 0 in the store, where the kernel has that epilogue
            if self.took(self.lib.fs2_op_gemm_gated(self.dt, x, w, bias, gate, gate_scale, y, M, N, Cin, taps, S or M, self.st()), "gemm_gated"):
                return y
            _lib.check(self.lib.fs2_op_gemm(self.dt, self.dt, x, w, bias, y, M, N, Cin, taps, S or M, 0, self.st()), None, "gemm")
            return self.gate_(y, gate, gate_scale)
        _lib.check(self.lib.fs2_op_gemm(self.dt, F32 if out_f32 else self.dt, x, w, bias, y, M, N, Cin, taps, S or M, int(relu), self.st()), None, "gemm")
        return y

    def gemm_relu_dropout(self, x, w, bias, M, N, Cin, taps, S, p, key):
        """dropout(relu(x W^T + bias)) - the mask of ``dropout(., p, key)`` - in one launch where the slab kernel runs the shape."""
        if p > 0 and self.fuse_ln_drop:
            y = self.act(M, N)
            if self.took(self.lib.fs2_op_gemm_relu_dropout(self.dt, x, w, bias, y, M, N, Cin, taps, S or M, p, C.c_uint64(self.seed),
                                                           C.c_uint64(key), self.st()), "gemm_relu_dropout"):
                return y
        return self.dropout(self.gemm(x, w, bias, M, N, Cin, taps=taps, S=S, relu=True), p, key)

    def gemm_ln_tape(self, x, w, bias, res, g, b, M, N, Cin, taps=1, S=None, relu=False, drop=None):
        """y = LayerNorm(z), z = act(x W^T + bias) [+ res], both stored, in ONE launch (the inference engine's fused GEMM +
        LayerNorm epilogue with a pre-norm store); None where that epilogue does not apply (N > 256, odd shapes, knob off).
        drop = (p, key): z = dropout(act(.)) + res with the mask of ``dropout(., p, key)`` (the residual sites in training mode)."""
        if not self.fuse_ln or N > 256:
            return None
        y, z = self.act(M, N), self.act(M, N)
        if drop is not None and drop[0] > 0:
            if not self.fuse_ln_drop:
                return None
            st_ = self.lib.fs2_op_gemm_ln_tape_dropout(self.dt, x, w, bias, res, g, b, y, z, M, N, Cin, taps, S or M, int(relu), drop[0],
                                                       C.c_uint64(self.seed), C.c_uint64(drop[1]), self.st())
        else:
            st_ = self.lib.fs2_op_gemm_ln_tape(self.dt, x, w, bias, res, g, b, y, z, M, N, Cin, taps, S or M, int(relu), self.st())
        return (y, z) if self.took(st_, "gemm_ln_tape") else None

    def layernorm(self, x, res, g, b, M, H, dot_w=None, dot_b=0.0, mask=None, want_y=True):
        y = self.act(M, H) if want_y else None
        pred = self.empty(M) if dot_w is not None else None
        _lib.check(self.lib.fs2_op_layernorm(self.dt, x, res, g, b, y, dot_w, dot_b, mask, pred, M, H, self.st()), None, "layernorm")
        return y, pred

    # ---- backward operators ----
    def bgemm(self, A, B, Cout, bias=None, **kw):
        """operands in A's dtype (both fp32 or both bf16); C fp32 or the activation dtype, by Cout's dtype"""
        d = _desc(self._dt(Cout), **kw)
        if A.dtype != B.dtype:
            raise TypeError(f"bgemm operands differ: {A.dtype} vs {B.dtype}")
        ws = self.ws("bgemm", int(self.lib.fs2_op_bgemm_ws_bytes(C.byref(d))))
        _lib.check(self.lib.fs2_op_bgemm(self._dt(A), C.byref(d), A, B, Cout, bias, ws, self.st()), None, "bgemm")
        return Cout

    def tn256(self, **kw):
        """does this bf16 product run on the 256 x 256 tile kernel (include/fs2.h fs2_op_bgemm_tn256)"""
        return bool(self.lib.fs2_op_bgemm_tn256(C.byref(_desc(F32, **kw))))

    @staticmethod
    def _dt(t):
        return F32 if t.dtype == torch.float32 else BF16

    def col_sum(self, x, out, M, N, seg=0, accumulate=True, scale=1.0, ldx=None):
        ws = self.ws("colsum", int(self.lib.fs2_op_col_sum_ws_bytes(M, N, seg)))
        _lib.check(self.lib.fs2_op_col_sum(self._dt(x), x, out, ws, M, N, ldx or N, seg, int(accumulate), scale, self.st()), None, "col_sum")

    def col_sums(self, part, M, ld, ga, na, gb, nb, gc=None, accumulate_c=True):
        """part is (M, ld): ga (na), gb (nb) += the sums of its first na, next nb columns - one launch where gb follows ga in the flat
        buffer (a bias behind its weight, a LayerNorm's beta behind its gamma) - and, where asked, gc += (or =) those of the columns left"""
        adjacent = gb.data_ptr() == ga.data_ptr() + 4 * na
        if adjacent and gc is not None:
            return self.col_sum2(part, ga, gc, na + nb, M, ld, accumulate2=accumulate_c)
        if adjacent:
            self.col_sum(part, ga, M, na + nb, ldx=ld)
        else:
            self.col_sum(part, ga, M, na, ldx=ld)
            self.col_sum(part[:, na:], gb, M, nb, ldx=ld)
        if gc is not None:
            self.col_sum(part[:, na + nb:], gc, M, ld - na - nb, ldx=ld, accumulate=accumulate_c)

    def col_sum2(self, x, out, out2, n1, M, N, ldx=None, accumulate=True, accumulate2=True):
        """columns [0, n1) of the sums to out, [n1, N) to out2"""
        ws = self.ws("colsum", int(self.lib.fs2_op_col_sum_ws_bytes(M, N, 0)))
        _lib.check(self.lib.fs2_op_col_sum2(self._dt(x), x, out, out2, n1, ws, M, N, ldx or N, int(accumulate), int(accumulate2), 1.0,
                                            self.st()), None, "col_sum2")

    def scatter_rows(self, x, idx32, idx64, table, R, H, V, skip_row):
        """embedding backward: table[idx[r]] += x[r]"""
        ws = self.ws("scatter", int(self.lib.fs2_op_scatter_rows_ws_bytes(R, H, V)))
        _lib.check(self.lib.fs2_op_scatter_rows(self._dt(x), x, idx32, idx64, table, ws, R, H, V, skip_row, self.st()), None,
                "scatter_rows")

    def relu_bwd(self, dy, y):
        """in place: dy *= (y > 0)"""
        self._guard(dy)
        _lib.check(self.lib.fs2_op_ew(self._dt(dy), 1, dy, y, dy, dy.numel(), 0, 0, self.st()), None, "relu_bwd")
        return dy

    def gate_(self, dy, y, scale=1.0):
        """in place: dy = y > 0 ? scale * dy : 0"""
        self.relu_bwd(dy, y)
        if scale != 1.0:
            _lib.check(self.lib.fs2_op_ew(self._dt(dy), 2, dy, None, dy, dy.numel(), scale, 0, self.st()), None, "scale")
        return dy

    def dwconv(self, x, w, bias, B, S, Cc, k):
        y = self.act(B * S, Cc)
        _lib.check(self.lib.fs2_op_dwconv(self.dt, x, w, bias, y, B, S, Cc, k, self.st()), None, "dwconv")
        return y

    def dwconv_bwd(self, du, x, w, gw, gb, B, S, Cc, k):
        """depth-wise conv backward: (gw (C, k), gb (C)) += the weight / bias gradients; returns d/dx (B*S, C)."""
        nparts = int(self.lib.fs2_op_dwconv_wgrad_parts(B, S))

        def wg():  # parameter gradients: a leaf (side stream where there is one)
            part = self.empty(nparts, Cc * (k + 1))
            _lib.check(self.lib.fs2_op_dwconv_wgrad(self.dt, du, x, part, B, S, Cc, k, self.st()), None, "dwconv_wgrad")
            self.col_sums(part, nparts, Cc * (k + 1), gw, Cc * k, gb, Cc)
        self.on_side((du, x), wg)
        dx = self.act(B * S, Cc)
        _lib.check(self.lib.fs2_op_dwconv_dgrad(self.dt, du, w, dx, B, S, Cc, k, self.st()), None, "dwconv_dgrad")
        return dx

    def dropout(self, x, p, key, out=None):
        """nn.Dropout (training): in place unless `out` is given; mask = f(self.seed, key, element index), so calling it again
        with the same key on a gradient is the backward."""
        if p <= 0.0:
            return x
        y = x if out is None else out
        self._guard(y)
        _lib.check(self.lib.fs2_op_dropout(self._dt(x), x, y, x.numel(), p, C.c_uint64(self.seed), C.c_uint64(key), self.st()), None, "dropout")
        return y

    def add_(self, a, b):
        self._guard(a)
        _lib.check(self.lib.fs2_op_ew(self._dt(a), 0, a, b, a, a.numel(), 1, 1, self.st()), None, "add")
        return a

    # y = x W^T + b backward pieces.  w is (N, taps*Cin) tap-major; x (M, Cin); dy (M, N); rows in utterances of S.
    def dgrad(self, dy, w, M, N, Cin, taps=1, S=None, out=None, accumulate=False, wt=None, gate=None, gate_scale=1.0):
        """dX (M, Cin) = dY (M, N) . W: with the transposed / tap-flipped copy wt (Cin, taps*N) through the forward
        GEMM / slab-conv kernel (dX is a 'same' conv of dY with wt), else through the strided-batched GEMM."""
        if out is not None:
            self._guard(out)
        if wt is not None and N % 64 == 0 and Cin % 64 == 0 and dy.dtype == wt.dtype:
            # a long reduction over few row tiles (encoder conv1: M = B L, K = taps x filter): K slices as workgroups of one launch
            # into fp32 planes, the plane sum folds the "+=" of an accumulating call (no separate add launch)
            ks = int(self.lib.fs2_op_gemm_splitk_choice(self.dt, M, Cin, N, taps, S or M)) if (gate is None and self.splitk) else 1
            if ks > 1:
                dx = out if out is not None else self.act(M, Cin)
                part = self.empty(ks, M, Cin)
                if self.took(self.lib.fs2_op_gemm_splitk(self.dt, self._dt(dx), dy, wt, dx, part, M, Cin, N, taps, S or M, ks,
                                                         int(bool(accumulate and out is not None)), self.st()), "gemm_splitk"):
                    return dx
            # out += dy . wt in the GEMM's own store (the accumulators start at out's tile)
            if out is not None and accumulate and gate is None and self.fuse_add and self.took(
                    self.lib.fs2_op_gemm_add(self.dt, dy, wt, None, out, out, M, Cin, N, taps, S or M, self.st()), "gemm_add"):
                return out
            dx = self.gemm(dy, wt, None, M, Cin, N, taps=taps, S=S, gate=gate, gate_scale=gate_scale)
            if out is None:
                return dx
            return self.add_(out, dx) if accumulate else out.copy_(dx)
        if gate is not None and (out is not None or accumulate):
            raise ValueError("dgrad: a gate goes with a fresh output only")
        dx = out if out is not None else self.act(M, Cin)
        beta = 1.0 if accumulate else 0.0
        if taps == 1:
            self.bgemm(dy, w, dx, M=M, N=Cin, K=N, sAm=N, sAk=1, sBk=Cin, sBn=1, ldc=Cin, beta=beta)
        else:
            pad = (taps - 1) // 2
            self.bgemm(dy, w, dx, M=M, N=Cin, K=taps * N, sAm=N, sAk=1, sBk=taps * Cin, sBn=1, ldc=Cin, seg=S or M,
                       taps=taps, Kin=N, a_shift0=pad, a_shift_step=-1, sBtap=Cin, beta=beta)
        return self.gate_(dx, gate, gate_scale) if gate is not None else dx

    def wgrad(self, dy, x, dw, db, M, N, Cin, taps=1, S=None, sync=False):
        """dw (N, taps*Cin) += dy^T x (per tap, rows shifted inside their utterance); db (N) += column sums of dy.
        ``sync``: the caller reads dw right away (the folded depth-wise conv2) - no side stream for this one."""
        if sync:
            return self._wgrad(dy, x, dw, db, M, N, Cin, taps, S)
        self.on_side((dy, x), lambda: self._wgrad(dy, x, dw, db, M, N, Cin, taps, S))

    def on_side(self, reads, fn):
        """Run the launches of fn() - LEAF work of the backward: parameter gradients nothing reads before the optimizer step - on the
        side stream, behind everything queued on the current stream so far; `reads` = the tensors they read."""
        if self.side is None:
            return fn()
        cur = torch.cuda.current_stream(self.dev)
        ready = torch.cuda.Event()
        ready.record(cur)                      # the inputs are complete on the main stream here
        self.side.wait_event(ready)
        self._ws_tag = "@side"
        try:
            with torch.cuda.stream(self.side):
                fn()
                done = torch.cuda.Event()
                done.record(self.side)
        finally:
            self._ws_tag = ""
        for t in reads:
            if t is not None:
                t.record_stream(self.side)     # the allocator must not hand the block out again before the side stream is through
                self._pending[self._base(t)] = done

    def _wgrad(self, dy, x, dw, db, M, N, Cin, taps=1, S=None):
        pad = (taps - 1) // 2
        kw = dict(M=N, N=Cin, K=M, sAm=1, sAk=N, sBk=Cin, sBn=1, ldc=taps * Cin, nb2=taps, sC2=Cin,
                  seg=(S or M) if taps > 1 else 0, b_shift0=-pad, b_shift_step=1, beta=1.0)
        if dy.dtype == torch.bfloat16 and self.tn256(**kw):
            # 256 x 256 tiles, one 512-thread workgroup per CU: fill the 256 CUs once (measured: conv1 7 splits = 252 workgroups,
            # 199 us against 335 on the 128 x 128 kernel; a second, part-filled round costs more than it brings)
            tiles = (N // 256) * (Cin // 256) * taps
            splitk = max(1, min(256 // tiles, 64, M // 256))
        else:
            tiles = ((N + 127) // 128) * ((Cin + 127) // 128) * taps
            splitk = max(1, min(32, -(-2304 // tiles), M // 1024))  # ~9 workgroups per CU (measured: conv1 16, conv2 / in-proj 32)
        self.bgemm(dy, x, dw, splitk=splitk, **kw)
        if db is not None:
            self.col_sum(dy, db, M, N)


class Trainer:
    """One process per GPU.  ``training_step(batch)`` = teacher-forced forward + losses + backward into the flat gradient
    buffer (accumulating, as Lightning's accumulate_grad_batches does); ``optimizer_step()`` = clip + AdamW + Noam."""

    def __init__(self, cfg: Fs2Config, state_dict, *, lr=2e-4, warmup_steps=4000, betas=(0.9, 0.98), eps=1e-8,
                 weight_decay=0.01, gradient_clip_val: Optional[float] = 1.0, variance_losses=None, mel_loss="l1",
                 duration_loss="mse", loss_alphas=None, precision="fp32", encoder_dropout=0.0, decoder_dropout=0.0,
                 variance_dropout=0.0, duration_dropout=0.0, seed=0, attention="auto", device="cuda:0",
                 soft_dtw_gamma=0.01, soft_dtw_chunk_size=256):
        # any mix of variance levels ("frame" / "phone") and transforms ("none" / "cwt"), as VarianceAdaptor.forward takes them
        # (model.py:276-333).  The reference's own FastSpeech2Loss reads self.mse_loss for a CWT variance's mean / std terms
        # (loss.py:141,148) and never sets it; plain nn.MSELoss() over the B utterance values is what the name stands for, and what
        # the fixtures were produced with (tools/gen_golden_train_variances.py).
        if cfg.duration_stochastic:  # its training forward is the flow's NLL with its own backward (sdp.py:276-331): inference only
            raise NotImplementedError("training step: a stochastic duration predictor (duration_stochastic=True) is not trained here")
        for i, v in enumerate(cfg.variances):
            # Fs2Config has already checked the level and transform names; the CWT head operators take these widths only
            if cfg.is_cwt(i) and (cfg.variance_filter_size % 64 or not 64 <= cfg.variance_filter_size <= 1024):
                raise ValueError(f"variance_filter_size = {cfg.variance_filter_size}: the CWT head of {v!r} trains with a multiple "
                                 f"of 64 up to 1024")
            if cfg.is_cwt(i) and variance_losses is not None and variance_losses[i] == "soft_dtw":
                # soft-DTW over a (B, S, 10) spectrogram is defined (loss.py:59-78) but has no fixture and no user: not built
                raise NotImplementedError(f"training step: 'soft_dtw' on the CWT variance {v!r} ('l1' / 'mse' on its spectrogram)")
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
        self.cfg, self.precision = cfg, precision
        self.ops = _Ops(device, precision)
        self.dev = self.ops.dev
        self.lr, self.warmup_steps, self.betas, self.eps, self.weight_decay = lr, warmup_steps, betas, eps, weight_decay
        # Lightning (>= 1.5, what the reference pins) reads gradient_clip_val None or 0 as "no clipping"; negative is an error there too
        if gradient_clip_val is not None and float(gradient_clip_val) < 0:
            raise ValueError(f"gradient_clip_val must be >= 0, got {gradient_clip_val}")
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val else None
        # 'same' padding of an even kernel is asymmetric (left (k-1)//2, right k-1-left): the data gradients run on the forward
        # kernels with tap-flipped weights, which is the transpose only for odd k (and the inference engine rejects even k too)
        for what, ks in (("encoder_kernel_sizes", cfg.encoder_kernel_sizes[:cfg.encoder_layers]),
                         ("decoder_kernel_sizes", cfg.decoder_kernel_sizes[:cfg.decoder_layers]),
                         ("variance_kernel_size", list(cfg.variance_kernel_size)), ("duration_kernel_size", [cfg.duration_kernel_size])):
            if any(int(k) % 2 == 0 for k in ks):
                raise ValueError(f"training step: {what} = {list(ks)} holds an even kernel size (odd sizes only, as in the inference engine)")
        # nn.Dropout sites of the reference in training mode (fastspeech2.py:94,103 encoder/decoder_dropout incl. the attention
        # weights and both PositionalEncoding calls; :65,74 variance / duration predictors).  Reference defaults 0.1 / 0.1 / 0.5 /
        # 0.5, the shipped recipe 0.1 everywhere (scripts/train.sh:12-13); 0 here unless asked, which is what parity pins.
        nv_ = len(cfg.variances)
        self.p_enc, self.p_dec, self.p_dur = float(encoder_dropout), float(decoder_dropout), float(duration_dropout)
        self.p_var = [float(v) for v in variance_dropout][:nv_] if isinstance(variance_dropout, (list, tuple)) else [float(variance_dropout)] * nv_
        self.seed, self._micro = int(seed), 0
        if attention not in ("auto", "materialized"):
            raise ValueError("attention must be 'auto' or 'materialized'")
        self.attention = attention  # auto: the fused forward + recomputing backward where built (bf16, head dim 128)
        self.variance_losses = list(variance_losses) if variance_losses is not None else ["mse"] * len(cfg.variances)
        self.mel_loss, self.duration_loss = mel_loss, duration_loss
        self.loss_alphas = dict(loss_alphas) if loss_alphas is not None else {
            "mel": 1.0, "pitch": 1e-1, "energy": 1e-1, "snr": 1e-1, "duration": 1e-4}
        missing = [k for k in ["mel", "duration"] + list(cfg.variances) if k not in self.loss_alphas]
        if missing:
            raise ValueError(f"loss_alphas has no entry for {missing} (the default covers mel / pitch / energy / snr / duration)")
        for k in self.variance_losses + [mel_loss, duration_loss]:
            if k not in _KIND and k != "soft_dtw":
                raise NotImplementedError(f"training step: loss kind {k!r} has no gradient kernel ('l1' / 'mse' / 'soft_dtw')")
        self.soft_dtw_gamma, self.soft_dtw_chunk_size = float(soft_dtw_gamma), int(soft_dtw_chunk_size)
        # ---- flat parameter / gradient / moment buffers, named views in KERNEL layout (conv weights tap-major) ----
        spec = state_dict_spec(cfg)
        self._layout: "OrderedDict[str, tuple]" = OrderedDict()   # name -> (offset, kernel shape, reference shape)
        off = 0
        for name, shape in spec.items():
            if name == "positional_encoding.pe" or name.endswith(".bins"):
                continue
            kshape = (shape[0], shape[2] * shape[1]) if len(shape) == 3 else tuple(shape)
            n = int(np.prod(shape))
            self._layout[name] = (off, kshape, tuple(shape))
            off += (n + 3) // 4 * 4  # every tensor starts on a 16-byte boundary
        self.n_flat = off
        self.flat_p = torch.zeros(off, device=self.dev)
        self.flat_g = torch.zeros(off, device=self.dev)
        self.flat_m = torch.zeros(off, device=self.dev)
        self.flat_v = torch.zeros(off, device=self.dev)
        self.P, self.G = self._views(self.flat_p), self._views(self.flat_g)
        # GEMM operands: the fp32 masters themselves, or their bf16 shadow (refreshed after every optimizer step)
        if self.ops.dt == F32:
            self.W = self.P
        else:
            self.flat_w = torch.zeros(off, device=self.dev, dtype=torch.bfloat16)
            self.W = self._views(self.flat_w)
        self.use_forward_dgrad = os.environ.get("FS2_TRAIN_DGRAD", "forward") == "forward"  # A/B switch: data gradients on the forward's GEMM / conv kernels ("bgemm": on the strided-batched GEMM)
        self.tw_batch = os.environ.get("FS2_TRAIN_TW_BATCH", "1") != "0"            # A/B switch: every weight transpose of a bf16 refresh in one launch
        self.adamw_shadow = os.environ.get("FS2_TRAIN_ADAMW_SHADOW", "1") != "0"    # A/B switch: the optimizer launch writes the bf16 shadow too
        # transposed, tap-flipped copies of every GEMM weight (activation dtype): the data gradients run on the forward kernels
        self.flat_wt = torch.zeros(off, device=self.dev, dtype=self.ops.tdt)
        self.WT = {}
        self._tw_table = None
        for n, wt in self._views(self.flat_wt).items():
            rs = self._layout[n][2]
            gemm_w = n.endswith("weight") and "embedding" not in n and (
                len(rs) == 2 or (len(rs) == 3 and rs[1] > 1 and ".conv2.0." not in n))  # not LayerNorm (1-D), depth-wise or grouped convs
            if gemm_w:
                self.WT[n] = wt.view(rs[1], -1)
        # depth-wise ConformerEncoderLayer: conv2 = grouped 1x1 + pointwise folded into one (H, F) map per optimizer step
        self.fold: Dict[str, dict] = {}
        H_ = cfg.hidden
        for side, nl, dw, F_ in (("encoder", cfg.encoder_layers, cfg.encoder_depthwise_conv, cfg.encoder_conv_filter_size),
                                 ("decoder", cfg.decoder_layers, cfg.decoder_depthwise_conv, cfg.decoder_conv_filter_size)):
            if dw:
                for i in range(nl):
                    self.fold[f"{side}.layers.{i}"] = {"Wf": self.ops.act(H_, F_), "bf": self.ops.empty(H_), "WfT": self.ops.act(F_, H_)}
        self.buffers: Dict[str, torch.Tensor] = {}
        self.load_state_dict(state_dict)
        self.steps = 0          # optimizer steps taken
        self._accum = 0         # micro-batches in the gradient buffer
        self._loss_ws = torch.zeros(int(self.ops.lib.fs2_op_masked_loss_ws_bytes()), dtype=torch.uint8, device=self.dev)
        self._nsq = torch.zeros(1, device=self.dev)
        self._nsq_ws = self.ops.empty(int(self.ops.lib.fs2_op_sum_sq_ws_bytes(off)) // 4 + 1)

    # ---- state ----
    def _views(self, flat):
        """name -> the parameter's part of a flat buffer, in kernel layout"""
        return {n: flat[o:o + math.prod(ks)].view(ks) for n, (o, ks, _) in self._layout.items()}

    def _to_kernel_layout(self, name, v, what):
        """a tensor or array in the reference's layout -> fp32 in the kernel's: conv weights (out, in, taps) tap-major, (out, taps * in)"""
        _, ks, rs = self._layout[name]
        t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(torch.float32)
        if tuple(t.shape) != rs:
            raise ValueError(f"{what}: shape {tuple(t.shape)} != {rs}")
        return (t.permute(0, 2, 1) if len(rs) == 3 else t).reshape(ks)

    def _to_ref_layout(self, name, t):
        """a view in the kernel's layout -> a host tensor in the reference's (the inverse of _to_kernel_layout)"""
        _, ks, rs = self._layout[name]
        t = t.detach().cpu()
        if len(rs) == 3:
            t = t.view(rs[0], rs[2], rs[1]).permute(0, 2, 1)
        return t.reshape(rs).contiguous()

    def _ref_views(self, flat):
        """name -> the parameter's part of a flat buffer, on the host in the reference's layout"""
        return OrderedDict((n, self._to_ref_layout(n, v)) for n, v in self._views(flat).items())

    def load_state_dict(self, sd):
        for name, p in self.P.items():
            p.copy_(self._to_kernel_layout(name, sd[name], name))
        for name in state_dict_spec(self.cfg):
            if name == "positional_encoding.pe" or name.endswith(".bins"):
                v = sd[name]
                t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(torch.float32)
                self.buffers[name] = t.reshape(-1, t.shape[-1]).contiguous().to(self.dev) if name.endswith(".pe") else t.contiguous().to(self.dev)
        self._refresh_shadow()

    def _refresh_shadow(self, converted=False):
        """bf16 weight shadow (unless the optimizer step has just written it), folded depth-wise conv2 maps, and the transposed
        tap-flipped weights the data gradients run on - all of those in one launch for bf16."""
        o = self.ops
        with torch.cuda.device(self.dev):
            if o.dt != F32 and not converted:
                _lib.check(o.lib.fs2_op_convert(F32, o.dt, self.flat_p, self.flat_w, self.n_flat, o.st()), None, "convert")
            for pfx, f in self.fold.items():
                Hh, Ff = f["Wf"].shape
                _lib.check(o.lib.fs2_op_fold_conv2(o.dt, self.P[f"{pfx}.conv2.0.weight"], self.P[f"{pfx}.conv2.0.bias"],
                                                   self.P[f"{pfx}.conv2.1.weight"], self.P[f"{pfx}.conv2.1.bias"], f["Wf"], f["bf"], Hh, Ff,
                                                   o.st()), None, "fold_conv2")
            jobs = [(f["Wf"], f["WfT"], f["Wf"].shape[0], f["Wf"].shape[1], 1) for f in self.fold.values()]
            if self.use_forward_dgrad:
                for n, wt in self.WT.items():
                    _, _, rs = self._layout[n]
                    jobs.append((self.W[n], wt, rs[0], rs[1], rs[2] if len(rs) == 3 else 1))
            if not jobs:
                return
            if o.dt == F32 or not self.tw_batch:
                for src, dst, N, Cin, taps in jobs:
                    _lib.check(o.lib.fs2_op_transpose_weight(o.dt, src, dst, N, Cin, taps, o.st()), None, "transpose_weight")
                return
            if self._tw_table is None:  # the buffers never move: build the device table once
                rows, tiles = [], 0
                for src, dst, N, Cin, taps in jobs:
                    rows.append([src.data_ptr(), dst.data_ptr(), N, Cin, taps, tiles])
                    tiles += int(o.lib.fs2_op_transpose_weight_tiles(N, Cin, taps))
                self._tw_table = (torch.tensor(rows, dtype=torch.int64, device=self.dev), len(rows), tiles)
            tab, n, tiles = self._tw_table
            _lib.check(o.lib.fs2_op_transpose_weight_batch(tab, n, tiles, o.st()), None, "transpose_weight_batch")

    def _wt(self, name):
        return self.WT.get(name) if self.use_forward_dgrad else None

    def state_dict(self):
        """Reference key names and layouts (feeds FastSpeech2(...) of this package or the reference's load_state_dict)."""
        out = self._ref_views(self.flat_p)
        for n, b in self.buffers.items():
            out[n] = b.cpu().reshape(1, *b.shape) if n.endswith(".pe") else b.cpu()
        return out

    def optimizer_state(self):
        """Adam moments under the reference's parameter names and layouts + the step counter (what a Lightning checkpoint keeps
        as ``optimizer_states`` / ``lr_schedulers``): ``{"step": n, "exp_avg": {name: tensor}, "exp_avg_sq": {name: tensor}}``.
        Together with ``state_dict()`` this resumes a run exactly."""
        return {"step": self.steps, "micro_step": self._micro, "exp_avg": self._ref_views(self.flat_m), "exp_avg_sq": self._ref_views(self.flat_v)}

    def load_optimizer_state(self, st):
        for key, flat in (("exp_avg", self.flat_m), ("exp_avg_sq", self.flat_v)):
            for n, view in self._views(flat).items():
                view.copy_(self._to_kernel_layout(n, st[key][n], f"{key}[{n}]"))
        self.steps = int(st["step"])
        self._micro = int(st.get("micro_step", 0))

    def lightning_optimizer_state(self):
        """``{"optimizer_states": [...], "lr_schedulers": [...]}`` in the layout Lightning writes for the reference's
        ``AdamW`` + ``NoamLR`` (fastspeech2.py:1166-1182): a checkpoint made of ``state_dict()`` + these two entries resumes in
        the reference, and ``load_lightning_optimizer_state`` resumes a reference checkpoint here."""
        from .checkpoint import to_lightning_optimizer_state
        out = to_lightning_optimizer_state(self.cfg, self.optimizer_state(), lr=self.lr, warmup_steps=self.warmup_steps,
                                           betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        out["fs2_micro_step"] = int(self._micro)  # the dropout-mask counter (Lightning keeps none): an extra key the reference ignores
        return out

    def load_lightning_optimizer_state(self, checkpoint, accumulate_grad_batches: int = 1):
        """``accumulate_grad_batches``: the value the run that wrote ``checkpoint`` was trained with (Lightning's Trainer flag,
        scripts/train.sh) - the dropout-mask counter resumes at optimizer steps x that many micro-batches, unless the checkpoint
        carries this framework's own ``fs2_micro_step`` (``lightning_optimizer_state()`` writes it)."""
        from .checkpoint import from_lightning_optimizer_state
        self.load_optimizer_state(from_lightning_optimizer_state(self.cfg, checkpoint, int(accumulate_grad_batches)))

    def gradients(self):
        return self._ref_views(self.flat_g)

    def zero_grad(self):
        self.flat_g.zero_()
        self._accum = 0

    def current_lr(self) -> float:
        """NoamLR.get_lr (noam.py:19-25) for the optimizer step about to be taken: last_epoch = steps taken so far."""
        e = max(1, self.steps)
        return self.lr * self.warmup_steps ** 0.5 * min(e ** -0.5, e * self.warmup_steps ** -1.5)

    # ---- forward / backward of one ConformerEncoderLayer (model.py:65-122, post-norm) ----
    def _layer_fwd(self, x, prefix, B, S, heads, F_, k, key_pad, pd=0.0):
        o, P, W, H = self.ops, self.P, self.W, self.cfg.hidden
        M, d = B * S, H // heads
        t = {"x": x, "pd": pd, "k_attn": o.site(), "k_sa": o.site(), "k_h": o.site(), "k_ff": o.site()}
        qkv = o.gemm(x, W[f"{prefix}.self_attn.in_proj_weight"], P[f"{prefix}.self_attn.in_proj_bias"], M, 3 * H, H)
        flash = self.attention == "auto" and bool(o.lib.fs2_op_attention_bwd_supported(o.dt, H, heads))
        scale = 1.0 / math.sqrt(d)
        attn = o.act(M, H)
        prob = prob_d = lse = None
        if flash:  # fused attention (scores never reach HBM) + lse2 for the recomputing backward
            bb = C.c_size_t()
            vb = int(o.lib.fs2_op_attention_scratch_bytes(o.dt, B, S, H, heads, C.byref(bb)))
            vt, bits = o.ws("attn_vt", vb), o.ws("attn_bits", int(bb.value))
            lse = o.empty(B, heads, S)
            _lib.check(o.lib.fs2_op_attention_train(o.dt, qkv, key_pad, attn, vt, bits, lse, B, S, H, heads, pd, C.c_uint64(o.seed),
                                                    C.c_uint64(t["k_attn"]), o.st()), None, "attention_train")
        else:
            scores = o.empty(B, heads, S, S)  # fp32 in either mode; the probabilities are kept in the activation dtype
            o.bgemm(qkv, qkv[:, H:], scores, M=S, N=S, K=d, sAm=3 * H, sAk=1, sBk=1, sBn=3 * H, ldc=S, nb1=B, nb2=heads,
                    sA1=S * 3 * H, sA2=d, sB1=S * 3 * H, sB2=d, sC1=heads * S * S, sC2=S * S)
            prob = scores if o.dt == F32 else o.act(B, heads, S, S)
            _lib.check(o.lib.fs2_op_softmax_fwd(o.dt, scores, key_pad, prob, B, heads, S, scale, o.st()), None, "softmax")
            del scores
            prob_d = o.dropout(prob, pd, t["k_attn"], out=o.act(B, heads, S, S)) if pd > 0 else prob  # MHA drops attention weights
            o.bgemm(prob_d, qkv[:, 2 * H:], attn, M=S, N=d, K=S, sAm=S, sAk=1, sBk=3 * H, sBn=1, ldc=H, nb1=B, nb2=heads,
                    sA1=heads * S * S, sA2=S * S, sB1=S * 3 * H, sB2=d, sC1=S * H, sC2=d)
        x1, proj, t["sum1"] = self._sublayer_fwd(attn, f"{prefix}.self_attn.out_proj", x, f"{prefix}.norm1", M, H, H, pd, t["k_sa"])  # dropout1
        if prefix in self.fold:  # depth-wise FFN (model.py:73-93): dw(k) -> pw H->F -> ReLU -> [grouped 1x1 . pw F->H] folded
            t["u"] = o.dwconv(x1, P[f"{prefix}.conv1.0.weight"], P[f"{prefix}.conv1.0.bias"], B, S, H, k)
            h = o.gemm_relu_dropout(t["u"], W[f"{prefix}.conv1.1.weight"], P[f"{prefix}.conv1.1.bias"], M, F_, H, 1, None, pd, t["k_h"])
            c2 = o.dropout(o.gemm(h, self.fold[prefix]["Wf"], self.fold[prefix]["bf"], M, H, F_), pd, t["k_ff"])
            t["sum2"] = False  # the folded map has no fused form: c2 is the summand, norm2 adds the residual
            x2, _ = o.layernorm(c2, x1, P[f"{prefix}.norm2.weight"], P[f"{prefix}.norm2.bias"], M, H)
        else:
            h = o.gemm_relu_dropout(x1, W[f"{prefix}.conv1.weight"], P[f"{prefix}.conv1.bias"], M, F_, H, k, S, pd, t["k_h"])
            x2, c2, t["sum2"] = self._sublayer_fwd(h, f"{prefix}.conv2", x1, f"{prefix}.norm2", M, H, F_, pd, t["k_ff"])  # dropout2
        t.update(qkv=qkv, prob=prob, prob_d=prob_d, lse=lse, key_pad=key_pad, attn=attn, proj=proj, x1=x1, h=h, c2=c2, scale=scale)
        return x2, t

    def _sublayer_fwd(self, x, lin, res, norm, M, N, Cin, p, key):
        """A residual sub-layer, z = res + dropout(x W^T + b) and y = LN(z), from the names of its linear map and its norm: ONE launch
        where the fused GEMM + LayerNorm epilogue takes the shape - it leaves the pre-norm sum for the tape too - else GEMM, dropout
        and the LayerNorm that adds the residual.  Returns (y, z, z_holds_residual): the stored z is the whole sum in the first case,
        the summand dropout(x W^T + b) in the second, and the backward's LayerNorm takes its residual accordingly."""
        o, P = self.ops, self.P
        w, b, g, beta = self.W[f"{lin}.weight"], P[f"{lin}.bias"], P[f"{norm}.weight"], P[f"{norm}.bias"]
        fused = o.gemm_ln_tape(x, w, b, res, g, beta, M, N, Cin, drop=(p, key))
        if fused is not None:
            return (*fused, True)
        z = o.dropout(o.gemm(x, w, b, M, N, Cin), p, key)
        return o.layernorm(z, res, g, beta, M, N)[0], z, False

    def _sublayer_bwd(self, dy, z, res, norm, db, M, H, p, key, accumulate=True):
        """Backward of _sublayer_fwd (res = None where z holds the residual): returns (the residual's gradient dz, the gradient of the
        sub-layer's output u = x W^T + b) and adds - or stores, for a scratch bias - u's bias gradient to db.  u's gradient is dz itself
        without dropout and the masked LayerNorm backward's second output with it; the bias gradient is then the third column block of
        that launch's partial sums.  With the fused dropout switched off: an explicit dropout pass and a column sum of its own."""
        o = self.ops
        fm = p > 0 and o.fuse_ln_drop
        if p <= 0 or fm:
            d = self._ln_bwd(z, res, dy, norm, M, H, bias_grad=db, bias_accumulate=accumulate, out_drop=(p, key) if fm else None)
            return d if fm else (d, d)
        dz = self._ln_bwd(z, res, dy, norm, M, H)
        du = o.dropout(dz, p, key, out=o.act(M, H))
        o.col_sum(du, db, M, H, accumulate=accumulate)
        return dz, du

    def _ln_bwd(self, z, res, dy, norm, M, H, bias_grad=None, bias_accumulate=True, relu_mask=False, drop=None, out_drop=None):
        """dz of y = LN(z [+ res]); dgamma / dbeta and, when asked, the bias gradient of the layer that produced z (= column sums of
        dz; with relu_mask dz is the pre-activation gradient) added to - or stored in - bias_grad.
        out_drop = (p, key): z = res + dropout(u) - returns (dz, dzm) with dzm = u's gradient (the mask applied in the same launch)
        and the bias gradient asked for is u's."""
        o = self.ops
        gname = f"{norm}.weight"
        nparts = int(o.lib.fs2_op_layernorm_bwd_parts(M))
        dz, part = o.act(M, H), o.empty(nparts, 3 * H)
        dzm = None
        if out_drop is not None and out_drop[0] > 0:
            dzm = o.act(M, H)
            _lib.check(o.lib.fs2_op_layernorm_bwd_masked(o.dt, z, res, dy, self.P[gname], dz, dzm, part, M, H, int(relu_mask), out_drop[0],
                                                         C.c_uint64(o.seed), C.c_uint64(out_drop[1]), o.st()), None, "layernorm_bwd")
        elif drop is not None and drop[0] > 0:  # dy is the gradient of dropout(y): the mask is applied on load, no separate pass
            _lib.check(o.lib.fs2_op_layernorm_bwd_dropout(o.dt, z, res, dy, self.P[gname], dz, part, M, H, int(relu_mask), drop[0],
                                                          C.c_uint64(o.seed), C.c_uint64(drop[1]), o.st()), None, "layernorm_bwd")
        else:
            _lib.check(o.lib.fs2_op_layernorm_bwd(o.dt, z, res, dy, self.P[gname], dz, part, M, H, int(relu_mask), o.st()), None, "layernorm_bwd")
        # (these column sums are leaves too, but on the side stream they measured SLOWER - 10.6 -> 11.0 ms per step: ~125 launches of
        # ~6 us each cost more in event records / waits than they free on the main chain; only the weight-gradient GEMMs go there)
        o.col_sums(part, nparts, 3 * H, self.G[gname], H, self.G[f"{norm}.bias"], H, bias_grad, bias_accumulate)
        return dz if dzm is None else (dz, dzm)

    def _layer_bwd(self, dx2, t, prefix, B, S, heads, F_, k):
        o, P, W, G, H = self.ops, self.P, self.W, self.G, self.cfg.hidden
        M, d = B * S, H // heads
        pd, folded = t["pd"], prefix in self.fold
        dbf = o.empty(H) if folded else None  # the folded map's bias gradient: stored, then unfolded into the conv2 pair's
        # x2 = LN2(x1 + dropout2(c2)): dz2 is the gradient of x1 (residual) and, through dropout2, of c2
        dx1, dc2 = self._sublayer_bwd(dx2, t["c2"], None if t["sum2"] else t["x1"], f"{prefix}.norm2",
                                      dbf if folded else G[f"{prefix}.conv2.bias"], M, H, pd, t["k_ff"], accumulate=not folded)
        if folded:
            f = self.fold[prefix]
            dWf = torch.zeros(H, F_, device=self.dev)
            o.wgrad(dc2, t["h"], dWf, None, M, H, F_, sync=True)
            _lib.check(o.lib.fs2_op_unfold_conv2(dWf, dbf, P[f"{prefix}.conv2.0.weight"], P[f"{prefix}.conv2.0.bias"],
                                                 P[f"{prefix}.conv2.1.weight"], G[f"{prefix}.conv2.0.weight"], G[f"{prefix}.conv2.0.bias"],
                                                 G[f"{prefix}.conv2.1.weight"], G[f"{prefix}.conv2.1.bias"], H, F_, o.st()), None, "unfold_conv2")
        # dh = (dc2 . W2) o [h > 0] / (1 - p): h = dropout(relu(.)) of the forward is > 0 exactly where the element was kept AND the
        # pre-activation was positive, so the ReLU backward and the dropout backward ride in the product's store together
        gate = t["h"] if o.gate else None
        gs = 1.0 / (1.0 - pd) if pd > 0 else 1.0
        if folded:
            dh = o.dgrad(dc2, f["Wf"], M, H, F_, wt=f["WfT"] if self.use_forward_dgrad else None, gate=gate, gate_scale=gs)
        else:
            o.wgrad(dc2, t["h"], G[f"{prefix}.conv2.weight"], None, M, H, F_)
            dh = o.dgrad(dc2, W[f"{prefix}.conv2.weight"], M, H, F_, wt=self._wt(f"{prefix}.conv2.weight"), gate=gate, gate_scale=gs)
        if gate is None:
            dh = o.relu_bwd(o.dropout(dh, pd, t["k_h"]), t["h"])  # h (post-dropout) > 0  <=>  kept and pre-activation > 0
        if folded:
            o.wgrad(dh, t["u"], G[f"{prefix}.conv1.1.weight"], G[f"{prefix}.conv1.1.bias"], M, F_, H)
            du = o.dgrad(dh, W[f"{prefix}.conv1.1.weight"], M, F_, H, wt=self._wt(f"{prefix}.conv1.1.weight"))
            o.add_(dx1, o.dwconv_bwd(du, t["x1"], P[f"{prefix}.conv1.0.weight"], G[f"{prefix}.conv1.0.weight"], G[f"{prefix}.conv1.0.bias"],
                                     B, S, H, k))
        else:
            o.wgrad(dh, t["x1"], G[f"{prefix}.conv1.weight"], G[f"{prefix}.conv1.bias"], M, F_, H, taps=k, S=S)
            o.dgrad(dh, W[f"{prefix}.conv1.weight"], M, F_, H, taps=k, S=S, out=dx1, accumulate=True, wt=self._wt(f"{prefix}.conv1.weight"))
        # x1 = LN1(x + dropout1(proj))
        dx, dproj = self._sublayer_bwd(dx1, t["proj"], None if t["sum1"] else t["x"], f"{prefix}.norm1",
                                       G[f"{prefix}.self_attn.out_proj.bias"], M, H, pd, t["k_sa"])
        o.wgrad(dproj, t["attn"], G[f"{prefix}.self_attn.out_proj.weight"], None, M, H, H)
        dattn = o.dgrad(dproj, W[f"{prefix}.self_attn.out_proj.weight"], M, H, H, wt=self._wt(f"{prefix}.self_attn.out_proj.weight"))
        qkv, prob = t["qkv"], t["prob"]
        dqkv = o.act(M, 3 * H)
        delta = o.empty(B, heads, S)
        _lib.check(o.lib.fs2_op_attn_delta(o.dt, dattn, t["attn"], delta, B, S, H, heads, o.st()), None, "attn_delta")
        if t["lse"] is not None:  # recomputing backward: P, dP, dS live in registers only
        # (its two launches - (dK, dV) and dQ - side by side on two streams measured nothing: 10.4-10.5 ms either way, r04)
            _lib.check(o.lib.fs2_op_attention_bwd(o.dt, qkv, dattn, t["lse"], delta, t["key_pad"], dqkv, B, S, H, heads, pd,
                                                  C.c_uint64(o.seed), C.c_uint64(t["k_attn"]), o.st()), None, "attention_bwd")
        else:
            bat = dict(nb1=B, nb2=heads)
            sP = dict(sA1=heads * S * S, sA2=S * S)
            # dV = dropout(P)^T dO
            o.bgemm(t["prob_d"], dattn, dqkv[:, 2 * H:], M=S, N=d, K=S, sAm=1, sAk=S, sBk=H, sBn=1, ldc=3 * H, sB1=S * H, sB2=d,
                    sC1=S * 3 * H, sC2=d, **bat, **sP)
            # dS = P o (dropout(dO V^T) - delta) / sqrt(d) in the product's epilogue: no dP tensor, no softmax-backward pass
            dp = o.act(B, heads, S, S)
            dsc = _desc(o.dt, M=S, N=S, K=d, sAm=H, sAk=1, sBk=1, sBn=3 * H, ldc=S, sA1=S * H, sA2=d, sB1=S * 3 * H, sB2=d,
                        sC1=heads * S * S, sC2=S * S, alpha=t["scale"], **bat)
            _lib.check(o.lib.fs2_op_bgemm_softmax_bwd(o.dt, C.byref(dsc), dattn, qkv[:, 2 * H:], dp, prob, delta, pd, C.c_uint64(o.seed),
                                                      C.c_uint64(t["k_attn"]), o.st()), None, "bgemm_softmax_bwd")
            # dQ = dS K ; dK = dS^T Q
            o.bgemm(dp, qkv[:, H:], dqkv, M=S, N=d, K=S, sAm=S, sAk=1, sBk=3 * H, sBn=1, ldc=3 * H, sB1=S * 3 * H, sB2=d,
                    sC1=S * 3 * H, sC2=d, **bat, **sP)
            o.bgemm(dp, qkv, dqkv[:, H:], M=S, N=d, K=S, sAm=1, sAk=S, sBk=3 * H, sBn=1, ldc=3 * H, sB1=S * 3 * H, sB2=d,
                    sC1=S * 3 * H, sC2=d, **bat, **sP)
        o.wgrad(dqkv, t["x"], G[f"{prefix}.self_attn.in_proj_weight"], G[f"{prefix}.self_attn.in_proj_bias"], M, 3 * H, H)
        o.dgrad(dqkv, W[f"{prefix}.self_attn.in_proj_weight"], M, 3 * H, H, out=dx, accumulate=True, wt=self._wt(f"{prefix}.self_attn.in_proj_weight"))
        return dx

    # ---- VariancePredictor (model.py:482-561, dense) ----
    def _predictor_fwd(self, x, prefix, nlayers, filt, k, B, S, mask, dw=False, pd=0.0, cwt=None):
        """cwt: the VarianceEncoder's prefix when the predictor ends in the CWT head (Linear(filter, 10) + mean_std_linear on the time
        mean of the last layer's output, model.py:413-415,508): pred is then (spec (M, 10), mean_std (B, 2)), both fp32."""
        o, P, W, H = self.ops, self.P, self.W, self.cfg.hidden
        M = B * S
        tape, y, cin = [], x, H
        for j in range(nlayers):
            p = f"{prefix}.layers.{j}.layers"
            u = None
            if dw:  # VarianceConvolutionLayer, depth-wise form (model.py:541-558): dw(k) -> pw 1x1 -> ReLU -> LN
                u = o.dwconv(y, P[f"{p}.0.module.0.weight"], P[f"{p}.0.module.0.bias"], B, S, cin, k)
                c = o.gemm(u, W[f"{p}.0.module.1.weight"], P[f"{p}.0.module.1.bias"], M, filt, cin, relu=True)
            last = j == nlayers - 1
            fl = None
            if not dw and pd <= 0 and not last:  # conv -> ReLU -> LayerNorm in one launch, the ReLU output kept for the tape
                fl = o.gemm_ln_tape(y, W[f"{p}.0.module.weight"], P[f"{p}.0.module.bias"], None, P[f"{p}.2.weight"], P[f"{p}.2.bias"],
                                    M, filt, cin, taps=k, S=S, relu=True)
            if fl is not None:
                yn, c = fl
                tape.append({"xin": y, "c": c, "cin": cin, "u": None, "kd": o.site()})
                y, cin = yn, filt
                continue
            if not dw:
                c = o.gemm(y, W[f"{p}.0.module.weight"], P[f"{p}.0.module.bias"], M, filt, cin, taps=k, S=S, relu=True)
            fused_head = last and pd <= 0 and cwt is None
            kd = None
            if pd > 0:  # VarianceConvolutionLayer ends in nn.Dropout (model.py:539,557): inside the LayerNorm launch
                kd = o.site()
                yn, pred = o.act(M, filt), None
                _lib.check(o.lib.fs2_op_layernorm_dropout(o.dt, c, None, P[f"{p}.2.weight"], P[f"{p}.2.bias"], yn, M, filt, pd,
                                                          C.c_uint64(o.seed), C.c_uint64(kd), o.st()), None, "layernorm_dropout")
            else:
                if fused_head:  # LayerNorm + the Linear(filter, 1) head + mask in one launch, the head's bias read on the device
                    yn, pred = o.act(M, filt), o.empty(M)
                    _lib.check(o.lib.fs2_op_layernorm_head(o.dt, c, None, P[f"{p}.2.weight"], P[f"{p}.2.bias"], yn,
                                                           P[f"{prefix}.linear.weight"], P[f"{prefix}.linear.bias"], mask, pred, M, filt,
                                                           o.st()), None, "layernorm_head")
                else:
                    yn, pred = o.layernorm(c, None, P[f"{p}.2.weight"], P[f"{p}.2.bias"], M, filt)
                kd = o.site()
            if last and pd > 0 and cwt is None:
                pred = o.empty(M)
                _lib.check(o.lib.fs2_op_row_dot(o.dt, yn, P[f"{prefix}.linear.weight"], P[f"{prefix}.linear.bias"], mask, pred, M, filt, o.st()), None, "row_dot")
            tape.append({"xin": y, "c": c, "cin": cin, "u": u, "kd": kd})
            y, cin = yn, filt
        ybar = None
        if cwt is not None:  # out_conv = y (behind the last layer's Dropout): ten dots per row + the utterance mean, one pass
            spec, ybar, ms = o.empty(M, 10), o.empty(B, filt), o.empty(B, 2)
            ws = o.ws("cwt_head", int(o.lib.fs2_op_cwt_head_train_ws_bytes(B, S, filt)))
            _lib.check(o.lib.fs2_op_cwt_head_train(o.dt, y, P[f"{prefix}.linear.weight"], P[f"{prefix}.linear.bias"],
                                                   P[f"{cwt}.mean_std_linear.weight"], P[f"{cwt}.mean_std_linear.bias"], mask, spec, ybar,
                                                   ms, ws, B, S, filt, o.st()), None, "cwt_head_train")
            pred = (spec, ms)
        return pred, {"layers": tape, "y": y, "pd": pd, "ybar": ybar}

    def _predictor_bwd(self, dpred, t, prefix, nlayers, filt, k, B, S, dx_out, dw=False, cwt=None):
        """dpred (M) - with the CWT head (cwt = the VarianceEncoder's prefix) the pair (dspec (M, 10), dmean_std (B, 2)) - ->
        gradients of the predictor's parameters, and dx_out (M, H) += d/dx."""
        o, P, W, G = self.ops, self.P, self.W, self.G
        M = B * S
        if cwt is not None:
            dspec, dms = dpred
            dy = o.act(M, filt)
            ws = o.ws("cwt_head_bwd", int(o.lib.fs2_op_cwt_head_bwd_ws_bytes(B, S, filt)))
            _lib.check(o.lib.fs2_op_cwt_head_bwd(o.dt, t["y"], dspec, dms, t["ybar"], P[f"{prefix}.linear.weight"],
                                                 P[f"{cwt}.mean_std_linear.weight"], dy, G[f"{prefix}.linear.weight"],
                                                 G[f"{prefix}.linear.bias"], G[f"{cwt}.mean_std_linear.weight"],
                                                 G[f"{cwt}.mean_std_linear.bias"], ws, B, S, filt, o.st()), None, "cwt_head_bwd")
            return self._predictor_layers_bwd(dy, t, prefix, nlayers, filt, k, B, S, dx_out, dw)
        # pred = y . w + b  (masked rows carry dpred = 0 already): dw = sum_m dpred[m] y[m] as a row-weighted column sum (fp32
        # weights; as a 1 x filt x M product on the 128 x 128 GEMM tile it took 51 us per head)
        ws = o.ws("colsum", int(o.lib.fs2_op_col_sum_ws_bytes(M, filt, 0)))
        _lib.check(o.lib.fs2_op_col_sum_weighted(o._dt(t["y"]), t["y"], dpred, G[f"{prefix}.linear.weight"], ws, M, filt, filt, 1, 1.0,
                                                 o.st()), None, "col_sum_weighted")
        dpred = o.to_act(dpred)
        o.col_sum(dpred, G[f"{prefix}.linear.bias"], M, 1)
        dy = o.act(M, filt)
        o.bgemm(dpred, W[f"{prefix}.linear.weight"], dy, M=M, N=filt, K=1, sAm=1, sAk=1, sBk=filt, sBn=1, ldc=filt)
        self._predictor_layers_bwd(dy, t, prefix, nlayers, filt, k, B, S, dx_out, dw)

    def _predictor_layers_bwd(self, dy, t, prefix, nlayers, filt, k, B, S, dx_out, dw):
        """dy (M, filt) = the gradient of the last layer's output -> the conv layers' gradients, dx_out (M, H) += d/dx"""
        o, P, W, G = self.ops, self.P, self.W, self.G
        M = B * S
        for j in reversed(range(nlayers)):
            p = f"{prefix}.layers.{j}.layers"
            lt = t["layers"][j]
            lin = f"{p}.0.module.1" if dw else f"{p}.0.module"  # the layer's GEMM: the point-wise conv behind the depth-wise one, or the conv
            # (the layer's Dropout behind its LayerNorm is undone inside the LayerNorm backward launch)
            dc = self._ln_bwd(lt["c"], None, dy, f"{p}.2", M, filt, bias_grad=G[f"{lin}.bias"], relu_mask=True, drop=(t["pd"], lt["kd"]))
            if dw:
                o.wgrad(dc, lt["u"], G[f"{lin}.weight"], None, M, filt, lt["cin"])
                du = o.dgrad(dc, W[f"{lin}.weight"], M, filt, lt["cin"], wt=self._wt(f"{lin}.weight"))
                dy = o.dwconv_bwd(du, lt["xin"], P[f"{p}.0.module.0.weight"], G[f"{p}.0.module.0.weight"], G[f"{p}.0.module.0.bias"],
                                  B, S, lt["cin"], k)
                if j == 0:
                    o.add_(dx_out, dy)
            else:  # the first layer's data gradient is added to dx_out in the product's own launch where that applies
                o.wgrad(dc, lt["xin"], G[f"{lin}.weight"], None, M, filt, lt["cin"], taps=k, S=S)
                dy = o.dgrad(dc, W[f"{lin}.weight"], M, filt, lt["cin"], taps=k, S=S, out=dx_out if j == 0 else None, accumulate=j == 0,
                             wt=self._wt(f"{lin}.weight"))

    def _loss_soft_dtw(self, name, pred, truth, truth_kind, mask, rows, inner):
        """get_loss with loss == "soft_dtw" (loss.py:62-81): pads zero-filled in prediction and target, the time axis cut into
        chunks of soft_dtw_chunk_size frames, soft-DTW of every (prediction chunk, target chunk) pair summed over chunks and batch;
        the gradient reaches the prediction only (truth.requires_grad = False, :63) and not its zero-filled pads.  Value and
        gradient of a chunk: fs2_op_soft_dtw_grad (csrc/softdtw.hip), pinned on the reference's vendored module."""
        from .softdtw import soft_dtw_value_and_grad
        Bm, Tm = mask.shape
        valid = (mask.view(Bm, Tm) == 0).unsqueeze(-1).to(torch.float32)
        p3 = pred.view(Bm, Tm, inner).to(torch.float32) * valid
        t3 = truth.view(Bm, Tm, -1).to(torch.float32) if truth_kind == 0 else torch.log(truth.view(Bm, Tm, 1).to(torch.float32) + 1)
        t3 = t3 * valid
        total = None
        grads = []
        for pc, tc in zip(p3.split(self.soft_dtw_chunk_size, dim=1), t3.split(self.soft_dtw_chunk_size, dim=1)):
            v, g = soft_dtw_value_and_grad(pc.contiguous(), tc.contiguous(), self.soft_dtw_gamma)
            total = v.sum() if total is None else total + v.sum()
            grads.append(g)
        dpred = (torch.cat(grads, dim=1) * valid * float(self.loss_alphas[name])).reshape(rows, inner) if inner > 1 else \
            (torch.cat(grads, dim=1) * valid * float(self.loss_alphas[name])).reshape(rows)
        return torch.stack([total, valid.sum() * inner]), dpred.contiguous()

    def _loss(self, name, pred, truth, truth_kind, mask, rows, inner, kind, want_grad=True):
        o = self.ops
        if kind == "soft_dtw":
            return self._loss_soft_dtw(name, pred, truth, truth_kind, mask, rows, inner)
        stat = o.empty(2)
        _lib.check(o.lib.fs2_op_masked_loss(pred, truth, truth_kind, mask, rows, inner, _KIND[kind], self._loss_ws, stat, o.st()), None, "masked_loss")
        dpred = None
        if want_grad:
            dpred = o.empty(rows, inner) if inner > 1 else o.empty(rows)
            _lib.check(o.lib.fs2_op_masked_loss_bwd(pred, truth, truth_kind, mask, stat, dpred, rows, inner, _KIND[kind],
                                                    self.loss_alphas[name], o.st()), None, "masked_loss_bwd")
        return stat, dpred

    # ---- the step ----
    def training_step(self, batch: dict) -> Dict[str, torch.Tensor]:
        """forward(targets, inference=False) + FastSpeech2Loss + backward; gradients are ADDED to the flat buffer.
        Returns the losses as 0-dim device tensors (same keys as the reference's loss dict)."""
        cfg, o, P, W, G, dev = self.cfg, self.ops, self.P, self.W, self.G, self.dev
        H = cfg.hidden
        phones = batch["phones"].to(dev, torch.int64).contiguous()
        dvec = batch["speaker"].to(dev, torch.float32).contiguous()
        dur_t = batch["duration"].to(dev, torch.int64).contiguous()
        mel_t = batch["mel"].to(dev, torch.float32).contiguous()
        B, L = phones.shape
        T = int(mel_t.shape[1])
        if tuple(dur_t.shape) != (B, L):
            raise ValueError(f"duration must be {(B, L)}, got {tuple(dur_t.shape)}")
        nv = len(cfg.variances)
        phone_vis = [vi for vi in range(nv) if cfg.is_phone_level(vi)]
        frame_vis = [vi for vi in range(nv) if not cfg.is_phone_level(vi)]

        def target(key, shape):
            if key not in batch:
                raise ValueError(f"the batch has no {key} (must be {shape})")
            t = batch[key]
            t = (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))).to(dev, torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{key} must be {shape}, got {tuple(t.shape)}")
            return t
        var_t, cwt_t = {}, {}
        for vi, v in enumerate(cfg.variances):
            S_ = L if cfg.is_phone_level(vi) else T  # a phone-level variance is (B, L), model.py:276-294
            if cfg.is_cwt(vi):  # teacher-forced with the raw signal, bucketised as log(signal) (model.py:418-419): torch.log on the
                # device tensor, as the inference path takes it (model.py of this package), so both paths pick the same buckets
                var_t[v] = torch.log(target(f"variances_{v}_signal", (B, S_)))
                cwt_t[v] = (target(f"variances_{v}_spectrogram", (B, S_, 10)), target(f"variances_{v}_mean", (B,)),
                            target(f"variances_{v}_std", (B,)))
            else:
                var_t[v] = target(f"variances_{v}", (B, S_))
        pe = self.buffers["positional_encoding.pe"]
        with torch.cuda.device(dev):
            # ---------------- forward ----------------
            o.seed, o._site = (self.seed * 1000003 + self._micro) & 0xFFFFFFFFFFFFFFFF, 0
            self._micro += 1
            pe_drop = self.p_enc > 0  # PositionalEncoding(dropout=encoder_dropout) serves both stacks (fastspeech2.py:296-298)
            k_pe_enc, k_pe_dec = o.site(), o.site()
            spk = o.empty(B, H)
            _lib.check(o.lib.fs2_op_spk_proj(dvec, P["speaker_embedding.projection.weight"], P["speaker_embedding.projection.bias"], spk, B,
                                             H, dvec.shape[1], o.st()), None, "spk_proj")
            x = o.act(B * L, H)
            src_mask = o.empty(B, L, dtype=torch.uint8)
            zero_spk = torch.zeros(B, H, device=dev) if pe_drop else None
            _lib.check(o.lib.fs2_op_embed(o.dt, phones, P["phone_embedding.weight"], pe, zero_spk if pe_drop else spk, x, src_mask, B, L, H,
                                          cfg.n_phones, o.st()), None, "embed")
            if pe_drop:  # x = dropout(E[phones] + pe) + spk   (model.py:53-55, fastspeech2.py:655-660)
                o.dropout(x, self.p_enc, k_pe_enc)
                _lib.check(o.lib.fs2_op_bucket_embed(o.dt, x, None, None, None, 0, 1, 0, None, spk, x, None, B, L, H, o.st()), None, "add_spk")
            enc_t = []
            for i in range(cfg.encoder_layers):
                x, t = self._layer_fwd(x, f"encoder.layers.{i}", B, L, cfg.encoder_head, cfg.encoder_conv_filter_size,
                                       cfg.encoder_kernel_sizes[i], src_mask, pd=self.p_enc)
                enc_t.append(t)
            prior_idx = {}
            for pr in cfg.priors:  # output = output + relu(Emb[bucketize(prior)]) per utterance (fastspeech2.py:687-692, model.py:160-164)
                pfx = f"prior_embeddings.{pr}"
                vals = torch.as_tensor(np.asarray(batch[f"priors_{pr}"].cpu() if isinstance(batch[f"priors_{pr}"], torch.Tensor)
                                                  else batch[f"priors_{pr}"]), dtype=torch.float32).to(dev).contiguous()
                if vals.numel() != B:
                    raise ValueError(f"priors_{pr} must hold one value per utterance")
                remb = o.empty(cfg.variance_nbins, H)
                _lib.check(o.lib.fs2_op_ew(F32, 1, P[f"{pfx}.embedding.weight"], P[f"{pfx}.embedding.weight"], remb, remb.numel(), 0, 0, o.st()), None, "relu")
                idx = o.empty(B * L, dtype=torch.int32)
                xn = o.act(B * L, H)
                _lib.check(o.lib.fs2_op_bucket_embed_utt(o.dt, x, vals, self.buffers[f"{pfx}.bins"], remb, cfg.variance_nbins, xn, idx, B,
                                                         L, H, o.st()), None, "prior_embed")
                prior_idx[pr] = idx.view(B, L)[:, 0].contiguous()
                x = xn
            dur_pred, dur_tape = self._predictor_fwd(x, "variance_adaptor.duration_predictor", cfg.duration_nlayers,
                                                     cfg.duration_filter_size, cfg.duration_kernel_size, B, L, src_mask,
                                                     dw=cfg.duration_depthwise_conv, pd=self.p_dur)
            var_pred, var_tape, var_idx = {}, {}, {}

            def variance_fwd(vi, xa, S_, mask, pe_, spk_):
                """VarianceEncoder.forward with its target (model.py:409-422): the prediction, and xa + Emb[bucketize(target)]"""
                v = cfg.variances[vi]
                pfx = f"variance_adaptor.encoders.{v}"
                var_pred[v], var_tape[v] = self._predictor_fwd(xa, f"{pfx}.predictor", cfg.variance_nlayers[vi], cfg.variance_filter_size,
                                                               cfg.variance_kernel_size[vi], B, S_, mask, dw=cfg.variance_depthwise_conv,
                                                               pd=self.p_var[vi], cwt=pfx if cfg.is_cwt(vi) else None)
                idx = o.empty(B * S_, dtype=torch.int32)
                xn = o.act(B * S_, H)
                st_ = {"std": 1.0, "mean": 0.0} if cfg.is_cwt(vi) else cfg.stats[v]  # log(signal) is bucketised as it is
                _lib.check(o.lib.fs2_op_bucket_embed_target(o.dt, xa, var_t[v], self.buffers[f"{pfx}.bins"], P[f"{pfx}.embedding.weight"],
                                                            cfg.variance_nbins, st_["std"], st_["mean"], pe_, spk_, xn, idx, B, S_, H,
                                                            o.st()), None, "bucket_embed_target")
                var_idx[v] = idx
                return xn
            # the duration predictor saw x as it is here; the phone-level variances follow in order, each on x + the earlier embeddings
            for vi in phone_vis:
                x = variance_fwd(vi, x, L, src_mask, None, None)
            forced = dur_t.to(torch.int32)
            dur, cum, totals, guard = (o.empty(B, L, dtype=torch.int32), o.empty(B, L, dtype=torch.int32),
                                       o.empty(B, dtype=torch.int32), o.empty(B, dtype=torch.int32))
            _lib.check(o.lib.fs2_op_durations(dur_pred, src_mask, forced, dur, cum, totals, guard, B, L, o.st()), None, "durations")
            xr = o.act(B * T, H)
            tgt_mask = o.empty(B, T, dtype=torch.uint8)
            _lib.check(o.lib.fs2_op_regulate(o.dt, x, cum, totals, xr, tgt_mask, B, L, T, H, o.st()), None, "regulate")
            xa = xr
            for vi in frame_vis:  # the last frame-level embedding launch also adds pe (and spk)
                last = vi == frame_vis[-1]
                xa = variance_fwd(vi, xa, T, tgt_mask, pe if last else None, spk if (last and not pe_drop) else None)
            if not frame_vis:
                xn = o.act(B * T, H)
                _lib.check(o.lib.fs2_op_bucket_embed(o.dt, xa, None, None, None, 0, 1, 0, pe, None if pe_drop else spk, xn, None, B, T, H, o.st()), None, "pe_spk")
                xa = xn
            y = xa
            if pe_drop:  # y = dropout(x + pe) + spk   (fastspeech2.py:705-718)
                o.dropout(y, self.p_enc, k_pe_dec)
                _lib.check(o.lib.fs2_op_bucket_embed(o.dt, y, None, None, None, 0, 1, 0, None, spk, y, None, B, T, H, o.st()), None, "add_spk")
            dec_t = []
            for i in range(cfg.decoder_layers):
                y, t = self._layer_fwd(y, f"decoder.layers.{i}", B, T, cfg.decoder_head, cfg.decoder_conv_filter_size,
                                       cfg.decoder_kernel_sizes[i], tgt_mask, pd=self.p_dec)
                dec_t.append(t)
            mel = o.gemm(y, W["linear.weight"], P["linear.bias"], B * T, cfg.n_mels, H, out_f32=True)
            # ---------------- losses + their gradients (loss.py:83-213) ----------------
            losses = {}
            dvar = {}
            alpha_of = {}
            for vi, (v, kind) in enumerate(zip(cfg.variances, self.variance_losses)):
                S_, mask = (L, src_mask) if cfg.is_phone_level(vi) else (T, tgt_mask)  # loss.py:123-130
                if not cfg.is_cwt(vi):
                    stat, dvar[v] = self._loss(v, var_pred[v], var_t[v], 0, mask, B * S_, 1, kind)
                    losses[v] = stat[0]
                    alpha_of[v] = self.loss_alphas[v]
                    continue
                # loss.py:133-154: the masked loss on the spectrogram, plain MSE over the B utterance values of mean and std
                (spec, ms), (spec_t, mean_t, std_t) = var_pred[v], cwt_t[v]
                stat, dspec = self._loss(v, spec, spec_t, 0, mask, B * S_, 10, kind)
                losses[f"{v}_cwt"] = stat[0]
                every = torch.zeros(B, dtype=torch.uint8, device=dev)
                dms = o.empty(B, 2)
                for col, (nm, tt) in enumerate((("mean", mean_t), ("std", std_t))):
                    stat, d = self._loss(v, ms[:, col].contiguous(), tt, 0, every, B, 1, "mse")
                    losses[f"{v}_{nm}"] = stat[0]
                    dms[:, col] = d
                dvar[v] = (dspec, dms)
                for sfx in ("cwt", "mean", "std"):
                    alpha_of[f"{v}_{sfx}"] = self.loss_alphas[v]  # loss.py:51-55
            stat, dmel = self._loss("mel", mel, mel_t, 0, tgt_mask, B * T, cfg.n_mels, self.mel_loss)
            losses["mel"] = stat[0]
            stat, ddur = self._loss("duration", dur_pred, dur_t, 1, src_mask, B * L, 1, self.duration_loss)
            losses["duration"] = stat[0]
            alpha_of.update(mel=self.loss_alphas["mel"], duration=self.loss_alphas["duration"])
            losses["total"] = sum(v * alpha_of[k] for k, v in losses.items())
            # ---------------- backward ----------------
            dmel = o.to_act(dmel)
            o.wgrad(dmel, y, G["linear.weight"], G["linear.bias"], B * T, cfg.n_mels, H)
            dy = o.dgrad(dmel, W["linear.weight"], B * T, cfg.n_mels, H)
            for i in reversed(range(cfg.decoder_layers)):
                dy = self._layer_bwd(dy, dec_t[i], f"decoder.layers.{i}", B, T, cfg.decoder_head, cfg.decoder_conv_filter_size,
                                     cfg.decoder_kernel_sizes[i])
            dspk = torch.zeros(B, H, device=dev)
            o.col_sum(dy, dspk, B * T, H, seg=T)  # decoder input = dropout(adaptor out + pe) + spk (fastspeech2.py:705-718)
            dx = o.dropout(dy, self.p_enc, k_pe_dec)
            def variance_bwd(vi, d, S_):
                """d = the gradient of x + embedding: scattered into the embedding table (a leaf: side stream), then d += the
                predictor's d/dx - x reached both the sum and the predictor"""
                v = cfg.variances[vi]
                pfx = f"variance_adaptor.encoders.{v}"
                o.on_side((d,), lambda: o.scatter_rows(d, var_idx[v], None, G[f"{pfx}.embedding.weight"], B * S_, H, cfg.variance_nbins, -1))
                self._predictor_bwd(dvar[v], var_tape[v], f"{pfx}.predictor", cfg.variance_nlayers[vi], cfg.variance_filter_size,
                                    cfg.variance_kernel_size[vi], B, S_, d, dw=cfg.variance_depthwise_conv,
                                    cwt=pfx if cfg.is_cwt(vi) else None)
            for vi in reversed(frame_vis):
                variance_bwd(vi, dx, T)
            dxe = o.act(B * L, H)
            _lib.check(o.lib.fs2_op_regulate_bwd(o.dt, dx, cum, dxe, B, L, T, H, o.st()), None, "regulate_bwd")
            # the phone-level tape, all residual adds onto dxe in ONE order (bit-equal reruns): the regulator's segment sums, then the
            # phone-level variances last to first, then the duration predictor (which saw the encoder output before any of them)
            for vi in reversed(phone_vis):
                variance_bwd(vi, dxe, L)
            self._predictor_bwd(ddur, dur_tape, "variance_adaptor.duration_predictor", cfg.duration_nlayers, cfg.duration_filter_size,
                                cfg.duration_kernel_size, B, L, dxe, dw=cfg.duration_depthwise_conv)
            if cfg.priors:
                seg = o.empty(B, H)
                o.col_sum(dxe, seg, B * L, H, seg=L, accumulate=False)
                for pr in cfg.priors:
                    pfx = f"prior_embeddings.{pr}"
                    tmp = torch.zeros(cfg.variance_nbins, H, device=dev)
                    o.scatter_rows(seg, prior_idx[pr], None, tmp, B, H, cfg.variance_nbins, -1)
                    o.relu_bwd(tmp, P[f"{pfx}.embedding.weight"])
                    o.add_(G[f"{pfx}.embedding.weight"], tmp)
            for i in reversed(range(cfg.encoder_layers)):
                dxe = self._layer_bwd(dxe, enc_t[i], f"encoder.layers.{i}", B, L, cfg.encoder_head, cfg.encoder_conv_filter_size,
                                      cfg.encoder_kernel_sizes[i])
            o.col_sum(dxe, dspk, B * L, H, seg=L)
            o.dropout(dxe, self.p_enc, k_pe_enc)
            o.on_side((dxe,), lambda: o.scatter_rows(dxe, None, phones, G["phone_embedding.weight"], B * L, H, cfg.n_phones, 0))
            o.relu_bwd(dspk, spk)  # spk = relu(W dvec + b), model.py:137-143
            o.wgrad(dspk, dvec, G["speaker_embedding.projection.weight"], G["speaker_embedding.projection.bias"], B, H, dvec.shape[1])
        o.join_side()  # the weight gradients of this micro-step are in the flat buffer before anything reads it
        self._accum += 1
        self.last = {"mel": mel.view(B, T, cfg.n_mels), "duration_prediction": dur_pred.view(B, L), "tgt_mask": tgt_mask.bool(),
                     "src_mask": src_mask.bool()}
        for vi, v in enumerate(cfg.variances):  # a CWT variance hands back what the reference's teacher-forced call does (model.py:443-451)
            S_ = L if cfg.is_phone_level(vi) else T
            self.last[f"variances_{v}"] = ({"spectrogram": var_pred[v][0].view(B, S_, 10), "mean": var_pred[v][1][:, 0],
                                            "std": var_pred[v][1][:, 1]} if cfg.is_cwt(vi) else var_pred[v].view(B, S_))
        return losses

    def optimizer_step(self, group=None):
        """clip_grad_norm_(gradient_clip_val) on the mean of the accumulated micro-batch gradients, AdamW, NoamLR.  With an
        initialised torch.distributed process group (one process per GPU, "nccl" = RCCL) the flat gradient buffer is summed
        over the ranks first and the 1 / world factor joins the gradient scale - DDP's gradient averaging."""
        if self._accum == 0:
            raise RuntimeError("optimizer_step before any training_step")
        o = self.ops
        lr = self.current_lr()
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            from .dist import all_reduce_gradients
            world = torch.distributed.get_world_size(group)
            if world > 1:
                all_reduce_gradients(self.flat_g, group)
        with torch.cuda.device(self.dev):
            nsq = None
            if self.gradient_clip_val is not None:
                _lib.check(o.lib.fs2_op_sum_sq(self.flat_g, self.n_flat, self._nsq_ws, self._nsq, o.st()), None, "sum_sq")
                nsq = self._nsq
            shadow = self.flat_w if o.dt != F32 and self.adamw_shadow else None
            _lib.check(o.lib.fs2_op_adamw_shadow(self.flat_p, self.flat_g, self.flat_m, self.flat_v, shadow, self.n_flat, lr, self.betas[0],
                                                 self.betas[1], self.eps, self.weight_decay, self.steps + 1, nsq,
                                                 self.gradient_clip_val or 0.0, 1.0 / (self._accum * world), o.st()), None, "adamw")
        self.steps += 1
        self.zero_grad()
        self._refresh_shadow(converted=shadow is not None)
        return lr
