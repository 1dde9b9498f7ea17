#!/usr/bin/env python
"""tests/golden/sdp/*.npz: what the REAL stochastic duration predictor of the reference returns (build container only, CPU).

    python tools/gen_golden_sdp.py [module] [spline] [e2e]

  module_n{1,2,3}.npz  StochasticDurationPredictorWrapper(n, 256, 256, 3, .)(x, pad, inference=True) under torch.manual_seed: the
                       noise it drew, logw of its float32 run, logw64 of the same module after .double() on the same draw (the
                       reference casts its float32 draw), and the ceil(exp(.)) durations.  B = 3, L = 150, lengths 150 / 1 / 75.
  spline.npz           ~2,000 (x1, h29) rows through piecewise_rational_quadratic_transform(inverse=True, tails="linear",
                       tail_bound=5) in float32 and float64: both tails, x1 = +-5, a float step inside and outside the bound,
                       every bin, values on interior knots.
  e2e_dense_small.npz  the dense_small-sized model with duration_stochastic=True through the unmodified
                       FastSpeech2.forward(inference=True) under torch.manual_seed.

Arrays and JSON only; weights and x are re-derived from the frozen recipe (tests/_sdp_ref.py, synth_state_dict) and sha-checked.
A fixture is refused (pick another seed) when a valid exp(logw64) lies within 5e-5 relative of an integer or a spline input's
float64 discriminant is below 1e-6: with that the tests need no near-tie allowance.

The fixtures live in their own directory because tests/_golden.py takes every tests/golden/*.npz for a forward fixture."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sdp_ref as R  # noqa: E402
from lightningfastspeech2_amd.weights import synth_inputs, synth_state_dict  # noqa: E402
from tools.ref_import import build_reference_model, load_reference  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "sdp")
TIE = 5e-5
MIN_DISC = 1e-6


def near_integer(logw64, valid):
    e = np.exp(np.asarray(logw64, np.float64))[valid]
    return bool((np.abs(e - np.rint(e)) <= TIE * e).any())


def wrapper_for(cfg, weights):
    m, _ = load_reference()
    w = m.StochasticDurationPredictorWrapper(cfg.duration_nlayers, cfg.hidden, cfg.duration_filter_size, cfg.duration_kernel_size, 0.5)
    w.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()}, strict=True)
    return w.eval()


@torch.no_grad()
def run_wrapper(w, x, pad, seed):
    B, L = pad.shape
    torch.manual_seed(seed)
    noise = torch.randn(B, 2, L)
    torch.manual_seed(seed)
    logw = w(torch.as_tensor(x), torch.as_tensor(pad), inference=True)
    torch.manual_seed(seed)
    logw64 = w.double()(torch.as_tensor(x).double(), torch.as_tensor(pad), inference=True)
    w.float()
    return noise.numpy(), logw.numpy(), logw64.numpy()


def gen_module():
    for n in (1, 2, 3):
        cfg = R.module_config(n)
        for seed in range(100 * n, 100 * n + 50):
            weights = R.sdp_state_dict(cfg, seed)
            x, pad = R.module_inputs(seed + 1)
            noise, logw, logw64 = run_wrapper(wrapper_for(cfg, weights), x, pad, seed + 2)
            if near_integer(logw64, ~pad):
                print(f"module n={n}: seed {seed} has a near-integer exp(logw64), next")
                continue
            d = np.ceil(np.exp(logw + np.float32(1e-9)))
            d[logw == 0] = 0
            d = np.clip(d, 0, None).astype(np.int32)
            d64 = np.ceil(np.exp(logw64))
            d64[logw64 == 0] = 0
            assert np.array_equal(d, d64.astype(np.int32)), "float32 and float64 durations differ although no tie is near"
            e_ref = float(np.abs(logw - logw64).max())
            np.savez_compressed(os.path.join(OUT_DIR, f"module_n{n}.npz"), config_json=cfg.to_json(),
                                recipe_json=json.dumps({"weights_seed": seed, "inputs_seed": seed + 1, "torch_seed": seed + 2}),
                                sha256=R.digest(weights, x, pad), noise=noise, logw=logw, logw64=logw64, durations=d)
            print(f"module n={n}: seed {seed}, logw in [{logw64.min():.3f}, {logw64.max():.3f}], e_ref {e_ref:.3e}, "
                  f"durations up to {d.max()}")
            break
        else:
            raise SystemExit(f"module n={n}: no seed without a near tie")


def spline_inputs(seed):
    rs = np.random.RandomState(seed)
    n_rand, n_knot = 1600, 200
    h = rs.standard_normal((n_rand + n_knot + 200, 29)).astype(np.float32)
    h[:, :20] *= 8.0  # divided by sqrt(256) = 16 inside: logits ~ N(0, 0.5^2)
    x = rs.uniform(-5.0, 5.0, n_rand).astype(np.float32)
    # values exactly on interior knots of the float32 cumulative heights (restated, tests/_sdp_ref.py)
    hk = torch.as_tensor(h[n_rand:n_rand + n_knot])
    uh = hk[:, 10:20] / 16.0
    s = 1e-3 + (1.0 - 1e-3 * 10) * torch.softmax(uh, -1)
    ch = torch.cumsum(s, -1) * 10.0 - 5.0
    knot = ch[torch.arange(n_knot), torch.as_tensor(rs.randint(0, 9, n_knot))].numpy().astype(np.float32)
    five = np.float32(5.0)
    edge = [five, -five, np.nextafter(five, np.float32(0)), np.nextafter(five, np.float32(10)),
            -np.nextafter(five, np.float32(0)), -np.nextafter(five, np.float32(10))]
    tails = np.concatenate([rs.uniform(5.0, 40.0, 70), -rs.uniform(5.0, 40.0, 70)]).astype(np.float32)
    special = np.concatenate([np.array(edge * 10, np.float32), tails])
    x = np.concatenate([x, knot, special]).astype(np.float32)
    assert len(x) == len(h), (len(x), len(h))
    return x, h


@torch.no_grad()
def gen_spline():
    load_reference()  # puts the reference on sys.path
    from litfass.third_party.stochastic_duration_predictor.transforms import piecewise_rational_quadratic_transform as prqt
    for seed in range(7, 40):
        x, h = spline_inputs(seed)

        def run(dt):
            xt, ht = torch.as_tensor(x).to(dt), torch.as_tensor(h).to(dt)
            out, _ = prqt(xt, ht[:, :10] / 16.0, ht[:, 10:20] / 16.0, ht[:, 20:], inverse=True, tails="linear", tail_bound=5.0)
            return out.numpy()
        _, disc, bins = R.spline_inverse(torch.as_tensor(x).double(), torch.as_tensor(h).double(), 16.0, return_details=True)
        hit = sorted(set(bins[bins >= 0].tolist()))
        assert hit == list(range(10)), f"spline: seed {seed} leaves bins unvisited: {hit}"
        if float(disc.min()) < MIN_DISC:
            print(f"spline: seed {seed} has a discriminant of {float(disc.min()):.2e}, next")
            continue
        out32, out64 = run(torch.float32), run(torch.float64)
        np.savez_compressed(os.path.join(OUT_DIR, "spline.npz"), recipe_json=json.dumps({"seed": seed, "F": 256}), x1=x, h29=h,
                            out32=out32, out64=out64)
        print(f"spline: seed {seed}, {len(x)} rows, e_ref {np.abs(out32 - out64).max():.3e}, min discriminant {float(disc.min()):.2e}, "
              f"rows per bin {np.bincount(bins[bins >= 0].numpy(), minlength=10).tolist()}")
        return
    raise SystemExit("spline: no seed with every discriminant above the floor")


def e2e_config():
    from tools.gen_golden import small
    # dense_small as it is (hidden 64), its duration predictor the flow predictor: 256 hidden channels, two flows
    return small(duration_stochastic=True, duration_depthwise_conv=False, duration_nlayers=2, duration_filter_size=256)


@torch.no_grad()
def gen_e2e():
    cfg = e2e_config()
    B, L, lengths = 3, 11, [11, 7, 4]
    for seed in range(300, 350):
        synth = dict(seed=seed, randomize_norm=True)
        sd = synth_state_dict(cfg, **synth)
        inp = synth_inputs(cfg, B, L, seed=seed + 1, lengths=lengths)
        model = build_reference_model(cfg, sd)
        enc = {}
        hook = model.variance_adaptor.duration_predictor.register_forward_hook(lambda mod, i, o: enc.__setitem__("x", i[0]))
        torch.manual_seed(seed + 2)
        noise = torch.randn(B, 2, L)
        torch.manual_seed(seed + 2)
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            out = model({"phones": torch.as_tensor(inp["phones"]), "speaker": torch.as_tensor(inp["speaker"])}, inference=True)
        hook.remove()
        pad = out["src_mask"].numpy()
        # the tie check on a float64 run of the predictor alone, fed the float32 encoder output the model produced
        w64 = R.sdp_weights(sd, torch.float64)
        logw64 = R.sdp_logw(w64, enc["x"].double(), pad, noise.double()).numpy()
        if near_integer(logw64, ~pad):
            print(f"e2e: seed {seed} has a near-integer exp(logw64), next")
            continue
        np.savez_compressed(os.path.join(OUT_DIR, "e2e_dense_small.npz"), config_json=cfg.to_json(), synth_json=json.dumps(synth),
                            recipe_json=json.dumps({"inputs_seed": seed + 1, "torch_seed": seed + 2, "lengths": lengths}),
                            sha256=R.digest({k: v for k, v in sd.items() if not k.endswith((".pe", ".bins"))}),
                            phones=inp["phones"], speaker=inp["speaker"], noise=noise.numpy(), logw64=logw64,
                            mel=out["mel"].numpy(), duration_prediction=out["duration_prediction"].numpy(),
                            duration_rounded=out["duration_rounded"].numpy().astype(np.int32), src_mask=pad,
                            tgt_mask=out["tgt_mask"].numpy())
        print(f"e2e: seed {seed}, T = {out['mel'].shape[1]}, durations {out['duration_rounded'].numpy().tolist()}")
        return
    raise SystemExit("e2e: no seed without a near tie")


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    what = sys.argv[1:] or ["module", "spline", "e2e"]
    if "module" in what:
        gen_module()
    if "spline" in what:
        gen_spline()
    if "e2e" in what:
        gen_e2e()
