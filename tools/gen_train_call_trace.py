#!/usr/bin/env python
"""The launch sequence of the training step, written down: every launch that one ``training_step`` + ``optimizer_step`` makes through
the C ABI, in order, with its arguments - tests/golden/train_call_trace.json, which tests/test_gpu_train_trace.py regenerates from the
working tree and compares for equality.  A refactor of lightningfastspeech2_amd/training.py must leave the file as it is; a change that
means to alter the launches regenerates it and shows the difference in its diff.
    python tools/gen_train_call_trace.py            (on the GPU; rewrites the fixture)

``Trainer.ops.lib`` is wrapped in a recording proxy (profiles/binding_call_cost.md counted calls the same way).  A launch is a call
whose last argument is a stream; host queries (``*_ws_bytes``, ``*_parts``, ``*_choice``, ``*_supported``, ``*_tn256``) take none, are
not recorded and may move.  One line per launch: the entry name, then each argument -
    ints, floats and c_uint64                                   by value
    a byref descriptor                                          {field=value, ...}, the non-zero fields in the header's order
    the stream                                                  main / side
    None                                                        None
    a tensor inside flat_p / flat_g / flat_w / flat_wt          p: / g: / w: / wt: + the parameter's name (+ the element offset into it,
                                                                if the tensor does not start where the parameter does); the whole
                                                                buffer by its letter alone
    any other tensor                                            dtype and shape, f32[39,64]
The cases are the small ones of tests/test_gpu_training.py and tests/test_gpu_training_variances.py: each in fp32 without dropout,
the WIDE (fused launches) and DW (depth-wise) ones again with every dropout site on, and once more in bf16 (side stream on)."""
import bisect
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
FIXTURE = os.path.join(ROOT, "tests", "golden", "train_call_trace.json")
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.int32: "i32", torch.int64: "i64", torch.uint8: "u8"}
_BYREF = type(C.byref(C.c_int()))


def cases():
    """id -> (cfg, state dict, batch, Trainer keywords)"""
    from test_gpu_training import DW, PRIORS, WIDE, _case
    from test_gpu_training_variances import CLASS_DEFAULT, SHAPES
    from _train_variances import case
    hyper = dict(lr=1e-3, warmup_steps=2, gradient_clip_val=0.5, variance_losses=["l1", "mse"], mel_loss="mse", duration_loss="l1")
    drop = dict(encoder_dropout=0.2, decoder_dropout=0.15, variance_dropout=[0.3, 0.25], duration_dropout=0.3, seed=9)
    shapes = {"base": (3, 4, 13, [13, 9, 5, 1], {}), "wide": (41, 3, 17, [17, 11, 4], WIDE), "dw": (5, 3, 21, [21, 8, 2], DW),
              "mixed": (6, 2, 9, [9, 4], dict(DW, decoder_depthwise_conv=False, variance_depthwise_conv=False)),
              "priors": (7, 3, 10, [10, 6, 8], PRIORS)}
    out = {}
    for name, (seed, B, L, lengths, kw) in shapes.items():
        out[f"{name}-fp32"] = (*_case(seed, B, L, lengths, **kw), hyper)
    assert SHAPES[0][4:6] == CLASS_DEFAULT  # phone-level pitch (CWT), energy and snr
    seed, B, L, lengths, levels, transforms, kw = SHAPES[0]
    out["phone_cwt-fp32"] = (*case(seed, B, L, lengths, levels, transforms, **kw), dict(hyper, variance_losses=["l1", "mse", "l1"]))
    for name in ("wide", "dw"):
        cfg, sd, batch, _ = out[f"{name}-fp32"]
        out[f"{name}-fp32-dropout"] = (cfg, sd, batch, dict(hyper, **drop))
        out[f"{name}-bf16"] = (cfg, sd, batch, dict(hyper, precision="bf16"))
    return out


class _Recorder:
    """stands in for Trainer.ops.lib: every entry point as it is, the launches written down as they are made"""

    def __init__(self, tr):
        self._lib, self._tr, self.lines = tr.ops.lib, tr, []
        self._starts = [o for o, _, _ in tr._layout.values()]
        self._names = list(tr._layout)
        self._flats = [(letter, getattr(tr, attr)) for letter, attr in (("p", "flat_p"), ("g", "flat_g"), ("w", "flat_w"), ("wt", "flat_wt"))
                       if hasattr(tr, attr)]

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            if args and hasattr(args[-1], "cuda_stream"):
                self.lines.append(" ".join([name] + [self._show(a) for a in args]))
            return fn(*args)
        return call

    def _show(self, a):
        if a is None or isinstance(a, (int, float)):
            return repr(a)
        if isinstance(a, C.c_uint64):
            return str(a.value)
        if isinstance(a, _BYREF):
            d = a._obj
            return "{" + ",".join(f"{f}={getattr(d, f)!r}" for f, _ in d._fields_ if getattr(d, f)) + "}"
        if hasattr(a, "cuda_stream"):
            side = self._tr.ops.side
            return "side" if side is not None and a.cuda_stream == side.cuda_stream else "main"
        if isinstance(a, torch.Tensor):
            for letter, flat in self._flats:
                off = a.data_ptr() - flat.data_ptr()
                if 0 <= off < flat.numel() * flat.element_size():
                    if off == 0 and a.numel() == flat.numel():
                        return letter
                    el = off // flat.element_size()
                    i = bisect.bisect_right(self._starts, el) - 1
                    return f"{letter}:{self._names[i]}" + (f"+{el - self._starts[i]}" if el != self._starts[i] else "")
            return f"{_DT[a.dtype]}[{','.join(map(str, a.shape))}]"
        return repr(a.item())  # a numpy scalar


def trace(cfg, sd, batch, kw):
    """the launches of one training_step + optimizer_step of a fresh Trainer, one line each"""
    from lightningfastspeech2_amd.training import Trainer
    tr = Trainer(cfg, sd, **kw)
    rec = tr.ops.lib = _Recorder(tr)
    tr.training_step({k: torch.as_tensor(v).cuda() for k, v in batch.items()})
    tr.optimizer_step()
    torch.cuda.synchronize()
    return rec.lines


def main():
    out = {name: trace(*c) for name, c in cases().items()}
    with open(FIXTURE, "w") as fh:  # one launch per line
        fh.write("{\n" + ",\n".join(f"{json.dumps(name)}: [\n" + ",\n".join(json.dumps(l) for l in lines) + "\n]"
                                    for name, lines in out.items()) + "\n}\n")
    print({name: len(lines) for name, lines in out.items()}, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
