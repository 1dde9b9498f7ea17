"""Test helper (CPU): the training step with phone-level and CWT variances as autograd over the forward oracle.

oracle/train_cpu.py restates the reference's FastSpeech2Loss for frame-level 'none' variances only; this restates
loss.py:83-213 for any level and for the CWT transform (a CWT variance v yields v_cwt on the (B, S, 10) spectrogram, masked,
and plain MSE v_mean / v_std over the B utterance values, each weighted with loss_alphas[v], loss.py:51-55), on top of
oracle_cpu.forward(..., teacher_targets=...).  Pinned on the fixtures the real reference produced
(tools/gen_golden_train_variances.py) by tests/test_train_variances_oracle.py."""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.weights import synth_state_dict
from oracle import oracle_cpu, train_cpu

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["train_phone_small", "train_cwt_small", "train_classdefault_small"]


def load_fixture(name):
    """(arrays, cfg, state dict, batch, hyper): <name>.npz plus its <name>.partN.npz side files as one mapping"""
    z = dict(np.load(os.path.join(GOLD_DIR, f"{name}.npz")))
    for i in range(int(z.get("n_parts", 0))):
        z.update(np.load(os.path.join(GOLD_DIR, f"{name}.part{i}.npz")))
    cfg = Fs2Config.from_json(str(z["config_json"]))
    skw = json.loads(str(z["synth_json"]))
    sd = synth_state_dict(cfg, skw.pop("seed"), **skw)
    batch = {k[3:]: z[k] for k in z if k.startswith("in_")}
    return _Arrays(z), cfg, sd, batch, json.loads(str(z["hyper_json"]))


class _Arrays(dict):
    """a dict with the .files of an NpzFile (what test_train_oracle.assert_params_close and the fixture loops read)"""

    @property
    def files(self):
        return list(self)


def _f(a):
    return torch.as_tensor(np.asarray(a)).float()


def losses(cfg, result, batch, variance_losses=None, mel_loss="l1", duration_loss="mse", loss_alphas=None):
    alphas = dict(train_cpu.DEFAULT_ALPHAS if loss_alphas is None else loss_alphas)
    kinds = variance_losses or ["mse"] * len(cfg.variances)
    tgt_valid, src_valid = ~result["tgt_mask"], ~result["src_mask"]
    out, weight = OrderedDict(), {}
    for vi, (v, kind) in enumerate(zip(cfg.variances, kinds)):
        valid = src_valid if cfg.is_phone_level(vi) else tgt_valid
        pred = result[f"variances_{v}"]
        if cfg.is_cwt(vi):
            out[f"{v}_cwt"] = train_cpu._masked(pred["spectrogram"], _f(batch[f"variances_{v}_spectrogram"]), kind, valid)
            out[f"{v}_mean"] = ((pred["mean"] - _f(batch[f"variances_{v}_mean"])) ** 2).mean()
            out[f"{v}_std"] = ((pred["std"] - _f(batch[f"variances_{v}_std"])) ** 2).mean()
            for s in ("cwt", "mean", "std"):
                weight[f"{v}_{s}"] = alphas[v]
        else:
            out[v] = train_cpu._masked(pred, _f(batch[f"variances_{v}"]), kind, valid)
            weight[v] = alphas[v]
    out["mel"] = train_cpu._masked(result["mel"], _f(batch["mel"]), mel_loss, tgt_valid)
    out["duration"] = train_cpu._masked(result["duration_prediction"], torch.log(_f(batch["duration"]) + 1), duration_loss, src_valid)
    weight.update(mel=alphas["mel"], duration=alphas["duration"])
    out["total"] = sum(v * weight[k] for k, v in out.items())
    return out


class VarianceOracleTrainer(train_cpu.OracleTrainer):
    """OracleTrainer with the level- and CWT-aware losses above"""

    def training_step(self, batch):
        tt = {k: batch[k] for k in batch if k == "duration" or k.startswith("variances_")}
        pri = {k: batch[k] for k in batch if k.startswith("priors_")}
        res = oracle_cpu.forward(self.sd, self.cfg, batch["phones"], batch["speaker"], teacher_targets=tt, priors=pri or None)
        ls = losses(self.cfg, res, batch, **self.loss_kw)
        ls["total"].backward()
        return {k: float(v.detach()) for k, v in ls.items()}, res


def check_grads(got, want, tol):
    assert sorted(got) == sorted(want)
    worst = ("", 0.0)
    for n, w in want.items():
        w = torch.as_tensor(w).float()
        err = float((torch.as_tensor(got[n]).float().cpu() - w).abs().max()) / (float(w.abs().max()) + 1e-3)
        if err > worst[1]:
            worst = (n, err)
    assert worst[1] <= tol, worst


def case(seed, B, L, lengths, levels, transforms, **kw):
    """a seeded configuration + batch with any mix of levels / transforms (modelled on tests/test_gpu_training.py:_case); teacher
    targets are drawn until they keep 1e-3 of a bin spacing from every bin edge"""
    from lightningfastspeech2_amd.weights import synth_inputs
    names = ["pitch", "energy", "snr"][:len(levels)]
    stats = {"pitch": {"min": 0.2, "max": 5.0, "mean": 0.1, "std": 1.5} if transforms[0] == "cwt" else {"min": -2.0, "max": 2.5, "mean": 0.1, "std": 1.5},
             "energy": {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0}, "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0}}
    base = dict(n_phones=30, encoder_hidden=64, decoder_hidden=64, encoder_head=2, decoder_head=4, encoder_layers=1,
                decoder_layers=2, encoder_kernel_sizes=[5], decoder_kernel_sizes=[9, 3], encoder_conv_filter_size=96,
                decoder_conv_filter_size=160, encoder_depthwise_conv=False, decoder_depthwise_conv=False,
                variance_filter_size=64, variance_depthwise_conv=False, variance_nlayers=[2, 1, 2][:len(levels)], variances=names,
                variance_levels=list(levels), variance_transforms=list(transforms), variance_kernel_size=[3, 5, 3][:len(levels)],
                duration_filter_size=64, duration_depthwise_conv=False, duration_nlayers=2, variance_nbins=24, n_mels=20, stats=stats)
    extra_stats = kw.pop("stats", None)
    base.update(kw)
    if extra_stats:
        base["stats"] = dict(stats, **{k: v for k, v in extra_stats.items() if k not in stats})
    cfg = Fs2Config(**base)
    sd = synth_state_dict(cfg, seed, randomize_norm=True, duration_bias=1.0)
    inp = synth_inputs(cfg, B, L, seed=seed + 1, lengths=lengths)
    rs = np.random.RandomState(seed + 2)
    dur = rs.randint(0, 5, size=(B, L)).astype(np.int64)
    for b, n in enumerate(lengths):
        dur[b, n:] = 0
    dur[0, 0] = max(1, dur[0, 0])
    T = int(dur.sum(1).max())
    batch = {"phones": inp["phones"], "speaker": inp["speaker"], "duration": dur, "mel": (rs.randn(B, T, cfg.n_mels) - 1.5).astype(np.float32)}
    batch.update({k: v for k, v in inp.items() if k.startswith("priors_")})
    for vi, v in enumerate(cfg.variances):
        S = L if cfg.is_phone_level(vi) else T
        bins = np.asarray(sd[f"variance_adaptor.encoders.{v}.bins"], dtype=np.float64)
        while True:
            t = np.exp(0.5 * rs.randn(B, S)).astype(np.float32) if cfg.is_cwt(vi) else (1.1 * rs.randn(B, S)).astype(np.float32)
            x = np.log(t.astype(np.float64)) if cfg.is_cwt(vi) else t.astype(np.float64) * cfg.stats[v]["std"] + cfg.stats[v]["mean"]
            if np.abs(x[..., None] - bins).min() >= 1e-3 * (bins[1] - bins[0]):
                break
        if cfg.is_cwt(vi):
            batch[f"variances_{v}_signal"] = t
            batch[f"variances_{v}_spectrogram"] = rs.randn(B, S, 10).astype(np.float32)
            batch[f"variances_{v}_mean"] = rs.randn(B).astype(np.float32)
            batch[f"variances_{v}_std"] = rs.uniform(0.5, 1.5, size=B).astype(np.float32)
        else:
            batch[f"variances_{v}"] = t
    return cfg, sd, batch
