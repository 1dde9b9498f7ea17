"""Teacher targets that replay a forward's own discrete decisions through the CPU oracle.

``oracle_cpu.forward(..., teacher_targets=teacher_targets(cfg, out))`` regulates with ``out["duration_rounded"]`` and bucketizes
every ``out["variances_<v>"]`` exactly as a prediction is bucketized (``bucketize(tgt * std + mean)``, right=False,
oracle_cpu.variance_encoder).  So the oracle runs under the decisions of whoever produced ``out`` (a GPU forward without debug taps
or forcing), and its own predictions and mel under those decisions can be compared with ``out``'s.

A CWT variance is teacher-forced with its raw signal, which a forward does not return: such configs are refused."""
import numpy as np
import torch


def teacher_targets(cfg, out) -> dict:
    bad = [v for i, v in enumerate(cfg.variances) if cfg.is_cwt(i)]
    if bad:
        raise ValueError(f"CWT variances {bad} are teacher-forced with their raw signal, which the forward does not return")

    def host(t):
        return t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
    tgt = {"duration": host(out["duration_rounded"]).long()}
    for v in cfg.variances:
        tgt[f"variances_{v}"] = host(out[f"variances_{v}"]).float()
    return tgt
