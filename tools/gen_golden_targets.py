#!/usr/bin/env python
"""tests/golden/frontend_targets.npz: what the REAL ``SNR.windowed_wada``, ``TTSDataset._create_variances`` and
``TTSDataset._interpolate`` of the reference return for a few synthetic utterances (build container only).  The reference's
``snr.py`` is loaded by path with an empty ``textgrid`` stub and registered as ``litfass.dataset.snr`` before ``datasets.py`` is
loaded, so ``_create_variances`` runs the real WADA code; every other absent third-party dependency is a stub module (none is
reached).  The fixture holds arrays and JSON only: the WADA table (the reference's data file), the waveforms, the outputs."""
import importlib
import importlib.util
import json
import os
import sys
import types
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REF)

STATS = {"snr": {"mean": 30.0, "std": 12.0}, "energy": {"mean": 0.1, "std": 0.08}, "pitch": {"mean": 150.0, "std": 40.0}}
# (n_fft = win_length, hop) and per utterance (samples, SNR in dB of the mix, seed)
CASES = {"default": ((1024, 256), [(16385, 20.0, 1), (9000, 0.0, 2), (4097, 60.0, 3), (1000, 35.0, 4), (12000, 10.0, 5)]),
         "small": ((256, 64), [(5000, 45.0, 6), (2049, 5.0, 7), (1000, 25.0, 8)])}


class Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return MagicMock()


def stub(name):
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        n = ".".join(parts[:i])
        if n not in sys.modules:
            m = Stub(n)
            m.__path__ = []
            sys.modules[n] = m


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def speech_like(n, snr_db, seed):
    """gamma-amplitude (shape 0.4, the WADA model) "speech" under a slow envelope + white Gaussian noise at snr_db; peak 1"""
    rs = np.random.RandomState(seed)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * np.arange(n) / 3000.0 + rs.uniform(0, 6.28))
    s = rs.gamma(0.4, 1.0, n) * rs.choice([-1.0, 1.0], n) * env
    noise = rs.standard_normal(n) * np.sqrt(np.mean(s ** 2) / 10.0 ** (snr_db / 10.0))
    x = (s + noise).astype(np.float32)
    return x / np.abs(x).max()


def phones_for(te, seed, shorter):
    """durations (>= 1 up front, so that the reference's in-place phone means read only original frames; a few zeros later) that
    sum to te, or to fewer frames when `shorter`; and the silent-phone flags"""
    rs = np.random.RandomState(100 + seed)
    total = te - (3 if shorter and te > 6 else 0)
    d = []
    while sum(d) < total:
        k = int(rs.randint(1, 7)) if len(d) < 3 or rs.rand() > 0.15 else 0
        d.append(min(k, total - sum(d)))
    d = np.asarray(d, np.int64)
    silent = rs.rand(len(d)) < 0.25
    if seed % 3 == 0:
        silent[0] = silent[-1] = True  # silence at both ends: the fill is the first / last present value
    return d, silent


def main():
    for n in ["textgrid"]:
        stub(n)
    for n in ["pyworld", "seaborn", "torchaudio", "torchaudio.transforms", "librosa", "librosa.filters", "pandarallel", "phones",
              "phones.convert", "srmrpy", "tqdm.rich", "PIL", "matplotlib", "matplotlib.pyplot", "matplotlib.gridspec",
              "litfass.dataset.cwt", "litfass.third_party.dvectors.wav2mel", "litfass.third_party.dvectors", "pytorch_lightning",
              "wandb", "rich", "g2p_en"]:
        try:
            importlib.import_module(n)
        except Exception:
            for k in [k for k in sys.modules if k == n or k.startswith(n + ".")]:
                del sys.modules[k]
            stub(n)
    snr_mod = load(os.path.join(REF, "litfass", "dataset", "snr.py"), "litfass.dataset.snr")
    old_err = np.geterr()
    try:
        ds = load(os.path.join(REF, "litfass", "dataset", "datasets.py"), "ref_datasets")  # sets np.seterr(... "raise") at import
        assert ds.SNR is snr_mod.SNR
        fix = {"wada_table": np.asarray(snr_mod.g_vals, np.float64)}
        meta = {"db_lo": -20, "stats": STATS, "cases": {}}
        for case, ((win, hop), utts) in CASES.items():
            meta["cases"][case] = {"n_fft": win, "win_length": win, "hop": hop, "utterances": []}
            for u, (n, snr_db, seed) in enumerate(utts):
                key = f"{case}__{u}"
                x = speech_like(n, snr_db, seed)
                te = -(-n // hop)
                d, silent = phones_for(te, seed, shorter=(u % 2 == 1))
                if case == "default" and u == 3:
                    silent[:] = True  # every frame silent: the all-missing fallback
                audio = torch.from_numpy(x.copy())
                frame_silent = ds.TTSDataset._expand(silent, d)
                fix[f"{key}__wav"] = x
                fix[f"{key}__duration"] = d
                fix[f"{key}__silent"] = silent
                fix[f"{key}__silence_mask"] = np.asarray(frame_silent, bool)
                fix[f"{key}__wada"] = np.asarray(snr_mod.SNR(x.copy(), 22050).windowed_wada(window=win, stride=hop / win, use_samples=True), np.float64)
                for level in ("frame", "phone"):
                    for with_stats in (False, True):
                        ns = SimpleNamespace(variances=["energy", "snr"], sampling_rate=22050, hop_length=hop, win_length=win,
                                             phone_level=level == "phone", variance_levels=[level, level],
                                             variance_transforms=["none", "none"])
                        if with_stats:
                            ns.stats = STATS
                        v = ds.TTSDataset._create_variances(ns, audio.clone(), frame_silent.copy(), d.copy())
                        tag = f"{key}__{level}__{'stats' if with_stats else 'raw'}"
                        fix[f"{tag}__snr"] = np.asarray(v["snr"], np.float64)
                        fix[f"{tag}__energy"] = np.asarray(v["energy"], np.float64)
                        if level == "frame" and not with_stats and not frame_silent.all():
                            # the prior of __getitem__ (datasets.py:435 with mean 0, std 1), formed from the reference's output
                            fix[f"{key}__prior_snr"] = np.asarray(np.mean(v["snr"][~frame_silent] * 1 + 0), np.float64)
                            fix[f"{key}__prior_energy"] = np.asarray(np.mean(v["energy"][~frame_silent] * 1 + 0), np.float64)
                if not silent.all():
                    fix[f"{key}__prior_duration"] = np.asarray(np.mean(d[~silent]), np.float64)
                # a synthetic F0 contour with unvoiced zeros through the reference's pitch lines (datasets.py:576-582)
                rs = np.random.RandomState(200 + seed)
                f0 = (120.0 + 40.0 * np.sin(np.arange(te) / 5.0) + rs.standard_normal(te)).astype(np.float32)
                f0[rs.rand(te) < 0.3] = 0.0
                if u == 2:
                    f0[:] = 0.0  # never voiced: the 1e-7 fallback
                fix[f"{key}__f0"] = f0.copy()
                p = f0.copy()
                p[p == 0] = np.nan
                if len(frame_silent) < len(p):
                    p = p[: sum(d)]
                p[frame_silent] = np.nan
                if np.isnan(p).all():
                    p[:] = 1e-7
                fix[f"{key}__pitch"] = np.asarray(ds.TTSDataset._interpolate(p), np.float64)
                meta["cases"][case]["utterances"].append({"samples": n, "snr_db": snr_db, "seed": seed, "frames": int(d.sum()), "windows": te})
    finally:
        np.seterr(**old_err)
    fix["meta_json"] = np.asarray(json.dumps(meta))
    path = os.path.join(ROOT, "tests", "golden", "frontend_targets.npz")
    np.savez_compressed(path, **fix)
    print(len(fix), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
