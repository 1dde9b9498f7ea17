#!/usr/bin/env python
"""tests/golden/fastdiff/fastdiff_{ragged,long,ragged_n68}.npz: what the REAL FastDiff of the reference returns (build container only,
CPU).

    python tools/gen_golden_fastdiff.py [ragged] [long] [ragged_n68]     (no name: all three)

A file whose recorded arrays come out bit for bit as they are on disk is left alone (a zip archive carries the time of writing).

The reference's default FastDiff() with lightningfastspeech2_amd.fastdiff.synth_state_dict(seed) loaded after remove_weight_norm, on
the synthetic mels of tests/_fastdiff_ref.fixture_mels:
  ragged  three utterances of 7, 4 and 1 frames, each run alone as generator.py:163-168 runs them
  long    one utterance of 70 frames
Per case: the mels, lengths, the handed-in noise (N = 4 draws per utterance; N = 3 uses the first three), eps of one forward at the
steps 74.99 and 498.05 of N = 4 (x = the utterance's x_T), inference(N = 4) and inference(N = 3) with the noise handed in, one seeded
run (torch.manual_seed, nothing handed in, utterance after utterance), the N = 3 / 4 schedules, and the state_dict's names and
shapes.  Every output is recorded twice over: float32 as the reference computes it, and the maximum absolute difference to a float64
run of the same modules on the same inputs (``*_err64``), the yardstick the tests derive their bounds from.  No weights: they are
regenerated from the seed.

  ragged_n68  the mels, lengths and weights of ``ragged`` under the two longer tabulated schedules: eight handed-in draws per
              utterance (N = 6 uses the first six), inference(N = 6) and inference(N = 8) with their ``_err64``, and the N = 6 / 8
              schedules.  A file of its own, so that the two above stay byte-identical.

std_normal is replaced while noise is handed in, and it hands in CLONES: sampling_given_noise_schedule updates its draw in place
(util.py:211, 228) and would otherwise corrupt the recorded input.

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

import _fastdiff_ref as R  # noqa: E402
from lightningfastspeech2_amd import fastdiff as FD  # noqa: E402
from tools.ref_import import REFERENCE_ROOT  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "fastdiff")
WEIGHT_SEED, RUN_SEED = 0, 1234
CASES = {"ragged": (11, [7, 4, 1]), "long": (12, [70])}


def reference_model(sd, double=False):
    sys.path.insert(0, REFERENCE_ROOT) if REFERENCE_ROOT not in sys.path else None
    import litfass.third_party.fastdiff.FastDiff as ref
    m = ref.FastDiff()
    m.remove_weight_norm()
    own = m.state_dict()
    assert sorted(own) == sorted(sd), "state_dict naming drifted"
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    m.eval()
    if double:
        m.double()
        emb = ref.calc_diffusion_step_embedding
        ref_double_emb = lambda *a, **k: emb(*a, **k).double()  # the float32 embedding of the float32 step, cast as the modules' dtype
        return m, ref, ref_double_emb
    return m, ref, None


class HandIn:
    """Replaces std_normal in the reference's modules: pops clones of the handed-in noise, in the reference's order of drawing."""

    def __init__(self, ref, dtype):
        import litfass.third_party.fastdiff.module.util as util
        self.mods, self.dtype, self.queue = (ref, util), dtype, []

    def __enter__(self):
        self.saved = [m.std_normal for m in self.mods]
        for m in self.mods:
            m.std_normal = lambda size, device="cpu": self.queue.pop(0).clone().to(self.dtype).view(size)
        return self

    def __exit__(self, *a):
        for m, f in zip(self.mods, self.saved):
            m.std_normal = f


@torch.no_grad()
def run_case(name, mel_seed, frames, sd):
    m32, ref, _ = reference_model(sd)
    m64, _, emb64 = reference_model(sd, double=True)
    mels = R.fixture_mels(mel_seed, frames)
    B, T = len(frames), max(frames)
    S = T * 256
    rs = np.random.RandomState(mel_seed + 100)
    noise = np.zeros((4, B, S), np.float32)
    for b, f in enumerate(frames):
        noise[:, b, :f * 256] = rs.standard_normal((4, f * 256)).astype(np.float32)
    out = {"mel": np.zeros((B, T, 80), np.float32), "lengths": np.asarray(frames, np.int32), "noise": noise}
    for b, f in enumerate(frames):
        out["mel"][b, :f] = mels[b]
    sched = {N: FD.inference_schedule(N, sqrt=torch.sqrt) for N in (3, 4)}  # the reference's own, with this host's torch.sqrt
    eps_steps = [float(sched[4]["steps"][2]), float(sched[4]["steps"][3])]
    out["eps_steps"] = np.asarray(eps_steps, np.float32)
    res = {k: np.zeros((B, S), np.float32) for k in ("eps_0", "eps_1", "wav_n4", "wav_n3", "wav_seeded")}
    err = {k: 0.0 for k in ("eps_0", "eps_1", "wav_n4", "wav_n3")}
    saved_emb = ref.calc_diffusion_step_embedding
    for b, f in enumerate(frames):
        n = f * 256
        c = torch.as_tensor(mels[b]).t().contiguous()  # (80, f)
        x = torch.as_tensor(noise[0, b, :n])
        for i, st in enumerate(eps_steps):
            ts = torch.full((1, 1), st, dtype=torch.float32)
            e32 = m32(x[None].clone(), c[None], ts).view(-1)
            ref.calc_diffusion_step_embedding = emb64
            e64 = m64(x[None].double(), c[None].double(), ts).view(-1)
            ref.calc_diffusion_step_embedding = saved_emb
            res[f"eps_{i}"][b, :n] = e32.numpy()
            err[f"eps_{i}"] = max(err[f"eps_{i}"], float((e32.double() - e64).abs().max()))
        for N in (4, 3):
            draws = [torch.as_tensor(noise[j, b, :n]) for j in range(N)]
            with HandIn(ref, torch.float32) as h:
                h.queue = list(draws)
                w32 = m32.inference(c.t(), N=N)  # (frames, 80), as generator.py:164-168 hands it over
                assert not h.queue
            with HandIn(ref, torch.float64) as h:
                h.queue = list(draws)
                ref.calc_diffusion_step_embedding = emb64
                w64 = m64.inference(c.t().double(), N=N)
                ref.calc_diffusion_step_embedding = saved_emb
            res[f"wav_n{N}"][b, :n] = w32.numpy()
            err[f"wav_n{N}"] = max(err[f"wav_n{N}"], float((w32.double() - w64).abs().max()))
    torch.manual_seed(RUN_SEED)
    for b, f in enumerate(frames):
        res["wav_seeded"][b, :f * 256] = m32.inference(torch.as_tensor(mels[b]), N=4).numpy()
    out.update(res)
    for k, v in err.items():
        out[k + "_err64"] = np.float64(v)
    for N in (3, 4):
        for k, v in sched[N].items():
            out[f"sched{N}_{k}"] = v.numpy()
    check_schedules(m32, sched, {4: [3.2176e-04, 2.5743e-03, 2.5376e-02, 7.0414e-01], 3: [9.0000e-05, 9.0000e-03, 6.0000e-01]})
    meta = {"weight_seed": WEIGHT_SEED, "run_seed": RUN_SEED, "mel_seed": mel_seed, "frames": frames,
            "config": {k: getattr(FD.FastDiffConfig(), k) for k in FD.FastDiffConfig.__dataclass_fields__},
            "state_dict": {k: list(v.shape) for k, v in m32.state_dict().items()},
            "eps_std": [float(res["eps_0"][b, :f * 256].std()) for b, f in enumerate(frames)]}
    out["meta"] = np.asarray(json.dumps(meta))
    save(name, out)
    print(name, {k: f"{v:.2e}" for k, v in err.items()}, "eps std", meta["eps_std"])


def check_schedules(m32, sched, betas):
    """the schedule as the reference's own sampler derives it (util.py:187-204), against inference_schedule(N, sqrt=torch.sqrt).  The
    recorded schedules are this host's: torch's CPU sqrt is not correctly rounded and differs between CPUs (inference_schedule's
    docstring), so regenerate on the host that recorded the committed files, or expect sched*_ and the waveforms to move."""
    import litfass.third_party.fastdiff.module.util as util
    for N, b in betas.items():
        a = 1 - torch.FloatTensor(b)
        for n in range(1, N):
            a[n] *= a[n - 1]
        a = torch.sqrt(a)
        steps = torch.FloatTensor([util.map_noise_scale_to_time_step(a[n], m32.diffusion_hyperparams["alpha"]) for n in range(N)])
        assert torch.equal(steps, sched[N]["steps"]) and torch.equal(a, sched[N]["alpha"]), (N, steps, sched[N]["steps"])


def save(name, out):
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, f"fastdiff_{name}.npz")
    if os.path.exists(path):
        old = np.load(path)
        if sorted(old.files) == sorted(out) and all(
                old[k].dtype == np.asarray(v).dtype and old[k].shape == np.asarray(v).shape and old[k].tobytes() == np.asarray(v).tobytes()
                for k, v in out.items()):
            print(name, "unchanged: file left as it is")
            return
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes written")


@torch.no_grad()
def run_n68(sd):
    """ragged_n68: the ragged utterances through the reference's inference(N = 6) and inference(N = 8), noise handed in"""
    mel_seed, frames = CASES["ragged"]
    m32, ref, _ = reference_model(sd)
    m64, _, emb64 = reference_model(sd, double=True)
    mels = R.fixture_mels(mel_seed, frames)
    B, T = len(frames), max(frames)
    S = T * 256
    rs = np.random.RandomState(mel_seed + 200)
    noise = np.zeros((8, B, S), np.float32)
    for b, f in enumerate(frames):
        noise[:, b, :f * 256] = rs.standard_normal((8, f * 256)).astype(np.float32)
    out = {"mel": np.zeros((B, T, 80), np.float32), "lengths": np.asarray(frames, np.int32), "noise": noise}
    for b, f in enumerate(frames):
        out["mel"][b, :f] = mels[b]
    sched = {N: FD.inference_schedule(N, sqrt=torch.sqrt) for N in (6, 8)}  # the reference's own, with this host's torch.sqrt
    check_schedules(m32, sched, {N: FD._BETAS[N] for N in (6, 8)})
    saved_emb = ref.calc_diffusion_step_embedding
    err = {}
    for N in (6, 8):
        wav = np.zeros((B, S), np.float32)
        err[N] = 0.0
        for b, f in enumerate(frames):
            n = f * 256
            c = torch.as_tensor(mels[b])  # (frames, 80), as generator.py:164-168 hands it over
            draws = [torch.as_tensor(noise[j, b, :n]) for j in range(N)]
            with HandIn(ref, torch.float32) as h:
                h.queue = list(draws)
                w32 = m32.inference(c, N=N)
                assert not h.queue
            with HandIn(ref, torch.float64) as h:
                h.queue = list(draws)
                ref.calc_diffusion_step_embedding = emb64
                w64 = m64.inference(c.double(), N=N)
                ref.calc_diffusion_step_embedding = saved_emb
                assert not h.queue
            wav[b, :n] = w32.numpy()
            err[N] = max(err[N], float((w32.double() - w64).abs().max()))
        out[f"wav_n{N}"] = wav
        out[f"wav_n{N}_err64"] = np.float64(err[N])
        for k, v in sched[N].items():
            out[f"sched{N}_{k}"] = v.numpy()
    meta = {"weight_seed": WEIGHT_SEED, "mel_seed": mel_seed, "noise_seed": mel_seed + 200, "frames": frames}
    out["meta"] = np.asarray(json.dumps(meta))
    save("ragged_n68", out)
    print("ragged_n68", {f"wav_n{N}": f"{v:.2e}" for N, v in err.items()})


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + ["ragged_n68"]
    sd = FD.synth_state_dict(FD.FastDiffConfig(), WEIGHT_SEED)
    for name in names:
        if name == "ragged_n68":
            run_n68(sd)
        else:
            run_case(name, *CASES[name], sd)
