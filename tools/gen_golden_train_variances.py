#!/usr/bin/env python
"""Golden vectors for the training step with phone-level and CWT variances: the REFERENCE itself (imported, build container
only, as tools/gen_golden_train.py does) - its teacher-forced FastSpeech2.forward(batch), its FastSpeech2Loss built with the
configuration's real variance_levels / variance_transforms, loss.backward(), clip_grad_norm_, AdamW and NoamLR, dropout off.

    python tools/gen_golden_train_variances.py [case ...]

    train_phone_small         config + weights of phone_teacher_small.npz   pitch phone, energy frame, snr phone
    train_cwt_small           config + weights of cwt_teacher_small.npz     frame-level CWT pitch
    train_classdefault_small  config + weights of phone_cwt_small.npz       phone-level CWT pitch, phone energy, frame snr

The reference's FastSpeech2Loss reads ``self.mse_loss`` for the CWT mean / std terms (loss.py:141,148) and never sets it; the
instance gets ``loss.mse_loss = nn.MSELoss()`` here (recorded in hyper_json as "reference_patch"), no reference file is touched.

Every teacher target is checked to lie at least MARGIN of the bin spacing away from its nearest bin edge (log(signal) for a
CWT variance, t * std + mean otherwise), so the bucket indices do not depend on the last ulp of ``log``; a seeded draw that
fails is drawn again with the next seed.

A fixture holds what train_small.npz holds plus ``param_order`` (the reference model's named_parameters() names in order).
The per-parameter arrays (grad_*, after3_*) are spread over side files <name>.partN.npz so that no file passes 1 MiB;
tests/_train_variances.py:load_fixture reads them back as one mapping."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightningfastspeech2_amd.config import Fs2Config  # noqa: E402
from lightningfastspeech2_amd.weights import synth_state_dict  # noqa: E402
from tools import ref_import  # noqa: E402
from tools.gen_golden_train import CLIP, LR, WARMUP  # noqa: E402

MARGIN = 1e-3
PART_BYTES = 900 * 1024
GOLD = os.path.join(ROOT, "tests", "golden")


def edge_margin(cfg, sd, vi, values, valid):
    """smallest distance of a (valid) teacher target to a bin edge, in units of the bin spacing"""
    v = cfg.variances[vi]
    bins = np.asarray(sd[f"variance_adaptor.encoders.{v}.bins"], dtype=np.float64)
    x = np.asarray(values, dtype=np.float64)
    with np.errstate(divide="ignore"):
        x = np.log(x) if cfg.is_cwt(vi) else x * cfg.stats[v]["std"] + cfg.stats[v]["mean"]
    d = np.abs(x[..., None] - bins).min(-1)
    return float(d[valid].min() / (bins[1] - bins[0]))


def draw(cfg, sd, vi, valid, seed, fn):
    """fn(RandomState) -> target; the first seed from `seed` on whose draw keeps MARGIN at EVERY position: a pad row can still
    receive gradient (a later predictor's conv backward spreads into it before this variance's embedding scatter)"""
    for s in range(seed, seed + 64):
        t = fn(np.random.RandomState(s))
        if edge_margin(cfg, sd, vi, t, np.ones_like(valid)) >= MARGIN:
            return t, s
    raise SystemExit(f"{cfg.variances[vi]}: no seed in [{seed}, {seed + 64}) keeps the bin-edge margin")


def save_parts(name, out):
    small = {k: v for k, v in out.items() if not k.startswith(("grad_", "after3_"))}
    parts, cur, size = [], {}, 0
    for k, v in out.items():
        if k in small:
            continue
        if size + v.nbytes > PART_BYTES and cur:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    if cur:
        parts.append(cur)
    small["n_parts"] = np.array(len(parts))
    paths = [(os.path.join(GOLD, f"{name}.npz"), small)] + [(os.path.join(GOLD, f"{name}.part{i}.npz"), p) for i, p in enumerate(parts)]
    for path, d in paths:
        np.savez_compressed(path, **d)
        kib = os.path.getsize(path) / 1024
        print(path, f"{kib:.1f} KiB")
        assert kib < 1024, path


def run_case(name, cfg, sd, synth_json, batch, FastSpeech2Loss, NoamLR, notes):
    model = ref_import.build_reference_model(cfg, sd)  # eval mode: dropout off
    nv = len(cfg.variances)
    loss = FastSpeech2Loss(variances=list(cfg.variances), variance_levels=list(cfg.variance_levels[:nv]),
                           variance_transforms=list(cfg.variance_transforms[:nv]), variance_losses=["mse"] * nv, mel_loss="l1",
                           duration_loss="mse", max_length=4096,
                           loss_alphas={"mel": 1.0, "pitch": 1e-1, "energy": 1e-1, "snr": 1e-1, "duration": 1e-4})  # the class default, own dict
    hyper = dict(lr=LR, warmup_steps=WARMUP, gradient_clip_val=CLIP)
    if any(cfg.is_cwt(i) for i in range(nv)):
        loss.mse_loss = torch.nn.MSELoss()
        notes = dict(notes, reference_patch="loss.mse_loss = nn.MSELoss()")
    opt = torch.optim.AdamW(model.parameters(), lr=LR, betas=[0.9, 0.98], eps=1e-8, weight_decay=0.01)
    sched = NoamLR(opt, WARMUP)
    out = {"config_json": np.array(cfg.to_json()), "synth_json": np.array(synth_json), "hyper_json": np.array(json.dumps(hyper)),
           "notes_json": np.array(json.dumps(notes)),
           "param_order": np.array([n for n, _ in model.named_parameters() if not n.startswith("fastdiff_linear")])}
    for k, v in batch.items():
        out["in_" + k] = v.numpy()
    for step in (1, 2, 3):
        np.random.seed(0)
        result = model(batch)
        losses = loss(result, batch)
        opt.zero_grad()
        losses["total"].backward()
        if step == 1:
            for k, v in losses.items():
                out[f"loss_{k}"] = np.float64(v.item())
            for n, p in model.named_parameters():
                if n.startswith("fastdiff_linear") or not p.requires_grad:
                    continue
                out["grad_" + n] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
        out[f"gradnorm_{step}"] = np.float64(float(norm))
        out[f"lr_{step}"] = np.float64(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        print(f"{name} step {step}: " + " ".join(f"{k}={float(v.detach()):.5f}" for k, v in losses.items()) + f" grad norm={float(norm):.4f}")
    for n, p in model.named_parameters():
        if not n.startswith("fastdiff_linear") and p.requires_grad:
            out["after3_" + n] = p.detach().numpy().copy()
    save_parts(name, out)


def build_batch(src, seed):
    """config + weights of tests/golden/<src>.npz; its tf_* teacher targets where it has them and they keep MARGIN, seeded ones else"""
    z = np.load(os.path.join(GOLD, f"{src}.npz"))
    cfg = Fs2Config.from_json(str(z["config_json"]))
    skw = json.loads(str(z["synth_json"]))
    sd = synth_state_dict(cfg, skw.pop("seed"), **skw)
    phones = z["phones"]
    B, L = phones.shape
    lengths = (phones != 0).sum(1)
    rs = np.random.RandomState(seed)
    if "tf_duration" in z.files:
        dur = z["tf_duration"].astype(np.int64)
    else:  # as train_dw_small
        dur = rs.randint(0, 6, size=(B, L)).astype(np.int64)
        for b, n in enumerate(lengths):
            dur[b, n:] = 0
    T = int(dur.sum(1).max())
    src_valid = phones != 0
    tgt_valid = np.arange(T)[None, :] < dur.sum(1)[:, None]
    batch = {"phones": phones, "speaker": z["speaker"], "duration": dur, "mel": (rs.randn(B, T, cfg.n_mels) * 1.3 - 2.0).astype(np.float32)}
    notes = {"source": src, "seed": seed, "targets": {}}
    for vi, v in enumerate(cfg.variances):
        S, valid = (L, src_valid) if cfg.is_phone_level(vi) else (T, tgt_valid)
        key = f"variances_{v}_signal" if cfg.is_cwt(vi) else f"variances_{v}"
        have = z["tf_" + key] if "tf_" + key in z.files else None
        if have is not None and have.shape == (B, S) and edge_margin(cfg, sd, vi, have, np.ones_like(valid)) >= MARGIN:
            batch[key], notes["targets"][key] = have, "golden"
        else:
            fn = (lambda r: np.exp(0.5 * r.randn(B, S)).astype(np.float32)) if cfg.is_cwt(vi) else (lambda r: (1.2 * r.randn(B, S)).astype(np.float32))
            batch[key], s = draw(cfg, sd, vi, valid, seed + 100 * (vi + 1), fn)
            notes["targets"][key] = f"seed {s}"
        notes["targets"][key + " margin"] = edge_margin(cfg, sd, vi, batch[key], valid)
        if cfg.is_cwt(vi):
            batch[f"variances_{v}_spectrogram"] = rs.randn(B, S, 10).astype(np.float32)
            batch[f"variances_{v}_mean"] = rs.randn(B).astype(np.float32)
            batch[f"variances_{v}_std"] = rs.uniform(0.5, 1.5, size=B).astype(np.float32)
    return cfg, sd, str(z["synth_json"]), {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in batch.items()}, notes


CASES = {"train_phone_small": ("phone_teacher_small", 781), "train_cwt_small": ("cwt_teacher_small", 782),
         "train_classdefault_small": ("phone_cwt_small", 783)}


def main():
    assert ref_import.reference_available(), "needs the reference checkout (build container only)"
    ref_import._install_stubs()
    sys.modules["pysdtw"].SoftDTW = lambda *a, **k: None
    from litfass.fastspeech2.loss import FastSpeech2Loss
    from litfass.fastspeech2.noam import NoamLR
    for name in (sys.argv[1:] or list(CASES)):
        src, seed = CASES[name]
        cfg, sd, synth_json, batch, notes = build_batch(src, seed)
        run_case(name, cfg, sd, synth_json, batch, FastSpeech2Loss, NoamLR, notes)


if __name__ == "__main__":
    main()
