#!/usr/bin/env python
"""Generate the fixtures of the two CPU tests that compare against the REAL reference on cases they build themselves
(build container only, where the reference can be imported):

    python tools/gen_golden_random.py

  tests/golden/random_reference.npz      what the unmodified reference forward returned for the ten randomised-hparams cases of
                                         tests/test_oracle_golden.py::test_oracle_matches_live_reference (per case: the config
                                         json, the sha256 of the synthetic weights, the inputs, the outputs)
  tests/golden/reference_param_order.json  named_parameters() order of the reference modules that
                                         tests/test_checkpoint_cpu.py::test_parameter_order_follows_the_reference_modules builds

The cases themselves (configs, weights, inputs) are built by the tests' own helpers; only inputs and outputs are stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.ref_import import load_reference, run_reference  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden")


def random_cases():
    from _golden import sd_digest
    from test_oracle_golden import N_RANDOM_CASES, random_case
    z = {}
    for seed in range(N_RANDOM_CASES):
        cfg, sd, inp = random_case(seed)
        ref = run_reference(cfg, sd, inp["phones"], inp["speaker"])
        z[f"s{seed}_config_json"] = np.array(cfg.to_json())
        z[f"s{seed}_sd_sha256"] = np.array(sd_digest(sd))
        z[f"s{seed}_phones"] = inp["phones"]
        for k in ["mel", "duration_prediction", "duration_rounded", "src_mask", "tgt_mask"] + [f"variances_{v}" for v in cfg.variances]:
            z[f"s{seed}_out_{k}"] = ref[k].detach().cpu().numpy()
    np.savez_compressed(os.path.join(OUT_DIR, "random_reference.npz"), **z)


def parameter_order():
    from test_checkpoint_cpu import _order_cfg
    cfg = _order_cfg()
    m, _ = load_reference()
    nv = len(cfg.variances)
    va = m.VarianceAdaptor(cfg.stats, list(cfg.variances), list(cfg.variance_levels[:nv]), list(cfg.variance_transforms[:nv]),
                           list(cfg.variance_nlayers[:nv]), list(cfg.variance_kernel_size[:nv]), [0.5] * nv, cfg.variance_filter_size,
                           cfg.variance_nbins, cfg.variance_depthwise_conv, cfg.duration_nlayers, False, cfg.duration_kernel_size, 0.5,
                           cfg.duration_filter_size, cfg.duration_depthwise_conv, cfg.hidden, 2756.25)
    names = {"config_json": cfg.to_json(), "variance_adaptor": [n for n, _ in va.named_parameters()]}
    for side, heads, F, k, dw in (("encoder", cfg.encoder_head, cfg.encoder_conv_filter_size, cfg.encoder_kernel_sizes[0], True),
                                  ("decoder", cfg.decoder_head, cfg.decoder_conv_filter_size, cfg.decoder_kernel_sizes[0], False)):
        layer = m.ConformerEncoderLayer(cfg.hidden, heads, conv_in=cfg.hidden, conv_filter_size=F, conv_kernel=(k, 1), batch_first=True,
                                        dropout=0.1, conv_depthwise=dw)
        names[f"{side}.layers.0"] = [n for n, _ in layer.named_parameters()]
    names["prior_embeddings.energy"] = [n for n, _ in m.PriorEmbedding(cfg.hidden, cfg.variance_nbins, cfg.stats["energy_prior"]).named_parameters()]
    names["speaker_embedding"] = [n for n, _ in m.SpeakerEmbedding(cfg.hidden, "dvector").named_parameters()]
    with open(os.path.join(OUT_DIR, "reference_param_order.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    random_cases()
    parameter_order()
