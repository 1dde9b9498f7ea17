"""Lightning-style checkpoints: a pickle written by torch.save of the dict Lightning writes - hyper_parameters
as pytorch_lightning's AttributeDict, state_dict of tensors, the on_save_checkpoint extras (fastspeech2.py:622-634) - read
back without Lightning installed, the class-default CWT pitch transform included, strict and tolerant loads."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from lightningfastspeech2_amd import checkpoint as ck
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.weights import state_dict_spec, synth_state_dict


def _cfg(**kw):
    base = dict(n_phones=30, encoder_hidden=32, decoder_hidden=32, encoder_head=2, decoder_head=2, encoder_layers=1,
                decoder_layers=1, encoder_kernel_sizes=[3], decoder_kernel_sizes=[3], encoder_conv_filter_size=64,
                decoder_conv_filter_size=64, variance_filter_size=32, variance_nlayers=[1, 1, 1], duration_filter_size=32,
                variance_nbins=8, n_mels=4, variance_transforms=["cwt", "none", "none"],
                stats={"pitch": {"min": 60.0, "max": 400.0, "mean": 180.0, "std": 40.0},
                       "energy": {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0},
                       "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0}})
    base.update(kw)
    return Fs2Config(**base)


def _write_lightning_checkpoint(path, cfg, sd, extra_state=None):
    """Pickle it the way Lightning does: hyper_parameters is an instance of
    pytorch_lightning.utilities.parsing.AttributeDict.  The class is provided by a throw-away module under that name and
    REMOVED again before loading, which is the situation of a machine without Lightning."""
    names = ["pytorch_lightning", "pytorch_lightning.utilities", "pytorch_lightning.utilities.parsing"]
    saved = {n: sys.modules.get(n) for n in names}
    mods = [types.ModuleType(n) for n in names]
    AD = type("AttributeDict", (dict,), {"__module__": names[2]})
    mods[2].AttributeDict = AD
    mods[0].utilities, mods[1].parsing = mods[1], mods[2]
    for n, m in zip(names, mods):
        sys.modules[n] = m
    try:
        hp = AD({k: v for k, v in cfg.to_dict().items() if k not in ("stats", "n_phones")})
        hp.update(lr=1e-4, warmup_steps=4000, fastdiff_variances=False, variance_dropout=[0.5, 0.5, 0.5])  # ignored extras
        ckpt = {"epoch": 3, "global_step": 1234, "pytorch-lightning_version": "1.5.10",
                "state_dict": {**{k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, **(extra_state or {})},
                "hyper_parameters": hp, "optimizer_states": [{"state": {}}], "lr_schedulers": [],
                "stats": cfg.stats, "phone2id": {f"p{i}": i for i in range(cfg.n_phones)},
                "speaker2dvector": {"spk0": np.zeros(256, np.float32)}, "speaker2priors": {"spk0": {"pitch": 1.0}}}
        torch.save(ckpt, path)
    finally:
        for n in names:
            if saved[n] is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = saved[n]


def test_reads_a_lightning_pickle_without_lightning(tmp_path):
    cfg = _cfg()
    sd = synth_state_dict(cfg, 3)
    path = tmp_path / "lit_model.ckpt"
    _write_lightning_checkpoint(path, cfg, sd, {"fastdiff_linear.0.weight": torch.zeros(32, 32)})
    assert "pytorch_lightning" not in sys.modules
    with pytest.raises(Exception):
        torch.load(path, map_location="cpu", weights_only=False)  # the stock loader cannot resolve AttributeDict
    c = ck.read_checkpoint(path)
    assert isinstance(c["hyper_parameters"], ck.AttributeDict) and c["hyper_parameters"].encoder_hidden == 32
    cfg2 = ck.config_from_checkpoint(c)
    assert cfg2.to_dict() == cfg.to_dict() and cfg2.is_cwt(0)  # the class default transform [cwt, none, none] survives
    w, rep = ck.resolve_state_dict(cfg2, c["state_dict"])
    assert set(w) == set(state_dict_spec(cfg)) and rep["dropped"] == ["fastdiff_linear.0.weight"]
    assert w["variance_adaptor.encoders.pitch.predictor.linear.weight"].shape == (10, 32)
    assert w["variance_adaptor.encoders.pitch.mean_std_linear.weight"].shape == (2, 32)
    for k in sd:
        np.testing.assert_array_equal(w[k], sd[k])


def test_strict_and_tolerant_loads(tmp_path, capsys):
    cfg = _cfg()
    sd = dict(synth_state_dict(cfg, 3))
    bad = dict(sd)
    bad["linear.weight"] = np.zeros((5, 32), np.float32)          # e.g. trained with another n_mels
    del bad["speaker_embedding.projection.bias"]
    with pytest.raises(ValueError, match="linear.weight"):
        ck.resolve_state_dict(cfg, bad)
    w, rep = ck.resolve_state_dict(cfg, bad, tolerant=True, init_seed=9)
    out = capsys.readouterr().out
    assert "Skip loading parameter: linear.weight, required shape: (4, 32), loaded shape: (5, 32)" in out  # fastspeech2.py:605-609
    assert rep == {"skipped": ["linear.weight"], "missing": ["speaker_embedding.projection.bias"], "dropped": []}
    fresh = synth_state_dict(cfg, 9)
    np.testing.assert_array_equal(w["linear.weight"], fresh["linear.weight"])  # keeps a fresh initialisation, as the reference
    np.testing.assert_array_equal(w["linear.bias"], sd["linear.bias"])


def test_opaque_lightning_objects_do_not_break_the_load(tmp_path):
    """a checkpoint may pickle instances of Lightning classes other than AttributeDict - enum members rebuilt as
    cls('fit'), callback / loop state objects with __setstate__.  Without Lightning they resolve to tolerant stand-ins."""
    import enum
    import pickle
    names = ["pytorch_lightning", "pytorch_lightning.trainer", "pytorch_lightning.trainer.states", "pytorch_lightning.callbacks"]
    saved = {n: sys.modules.get(n) for n in names}
    mods = [types.ModuleType(n) for n in names]
    Stage = enum.Enum("RunningStage", {"TRAINING": "train", "FITTING": "fit"}, module=names[2])
    mods[2].RunningStage = Stage

    class ProgressState:
        def __init__(self, a, b=2):
            self.a, self.b = a, b

        def __reduce__(self):
            return (ProgressState, (self.a,), {"b": self.b, "extra": [1, 2, 3]})
    ProgressState.__module__, ProgressState.__qualname__ = names[3], "ProgressState"
    mods[3].ProgressState = ProgressState
    for n, m in zip(names, mods):
        sys.modules[n] = m
    path = tmp_path / "odd.ckpt"
    try:
        torch.save({"state_dict": {"w": torch.ones(2)}, "stage": Stage.FITTING, "callbacks": {"progress": ProgressState(7)},
                    "loops": [ProgressState(1), ProgressState(2)]}, path)
    finally:
        for n in names:
            if saved[n] is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = saved[n]
    c = ck.read_checkpoint(path)
    assert torch.equal(c["state_dict"]["w"], torch.ones(2))
    assert c["stage"]._args == ("fit",)                      # the enum member's value survives for inspection
    assert c["callbacks"]["progress"]._args == (7,) and c["callbacks"]["progress"].b == 2
    assert [o._args for o in c["loops"]] == [(1,), (2,)]
    del pickle


def _order_cfg():
    return _cfg(priors=["energy", "duration"], encoder_depthwise_conv=True, decoder_depthwise_conv=False,
                stats={"pitch": {"min": 60.0, "max": 400.0, "mean": 180.0, "std": 40.0},
                       "energy": {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0}, "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0},
                       "energy_prior": {"min": -1.0, "max": 1.0, "mean": 0.0, "std": 1.0},
                       "duration_prior": {"min": 0.0, "max": 9.0, "mean": 3.0, "std": 1.0}})


def test_parameter_order_follows_the_reference_modules():
    """optimizer.state_dict() numbers parameters in FastSpeech2.parameters() order: module registration order of
    fastspeech2.py:242-438 (phone_embedding, encoder, variance_adaptor, decoder, linear, prior_embeddings, speaker_embedding),
    in-module order = the real modules' named_parameters() (tests/golden/reference_param_order.json, tools/gen_golden_random.py)."""
    cfg = _order_cfg()
    order = ck.parameter_order(cfg)
    tops = [n.split(".")[0] for n in order]
    firsts = [t for i, t in enumerate(tops) if i == 0 or tops[i - 1] != t]
    assert firsts == ["phone_embedding", "encoder", "variance_adaptor", "decoder", "linear", "prior_embeddings", "speaker_embedding"]
    assert "positional_encoding.pe" not in order and "variance_adaptor.encoders.pitch.bins" in order  # bins are frozen Parameters
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_param_order.json")) as f:
        ref = json.load(f)
    assert ref.pop("config_json") == cfg.to_json(), "config drifted from the fixture"
    assert set(ref) == {"variance_adaptor", "encoder.layers.0", "decoder.layers.0", "prior_embeddings.energy", "speaker_embedding"}
    for prefix, names in ref.items():
        assert [n for n in order if n.startswith(prefix + ".")] == [f"{prefix}.{n}" for n in names], prefix


def test_optimizer_state_round_trips_through_lightning_layout():
    """Trainer.optimizer_state() -> Lightning's optimizer_states / lr_schedulers -> a REAL torch.optim.AdamW over parameters in
    parameter_order accepts it, steps, and its state comes back unchanged through the inverse."""
    cfg = _cfg(variance_transforms=["none", "none", "none"])
    names = ck.parameter_order(cfg)
    spec = state_dict_spec(cfg)
    g = torch.Generator().manual_seed(0)
    train = [n for n in names if not n.endswith(".bins")]
    st = {"step": 17, "micro_step": 0, "exp_avg": {n: torch.randn(spec[n], generator=g) for n in train},
          "exp_avg_sq": {n: torch.rand(spec[n], generator=g) for n in train}}
    lit = ck.to_lightning_optimizer_state(cfg, st, lr=1e-3, warmup_steps=4000)
    params = [torch.nn.Parameter(torch.zeros(spec[n]), requires_grad=not n.endswith(".bins")) for n in names]
    opt = torch.optim.AdamW(params, lr=1e-3, betas=[0.9, 0.98], eps=1e-8, weight_decay=0.01)
    opt.load_state_dict(lit["optimizer_states"][0])          # torch's own shape / group validation
    for i, n in enumerate(names):
        if n.endswith(".bins"):
            assert params[i] not in opt.state
            continue
        assert torch.equal(opt.state[params[i]]["exp_avg"], st["exp_avg"][n])
        assert int(opt.state[params[i]]["step"]) == 17
    assert abs(opt.param_groups[0]["lr"] - 1e-3 * 4000 ** 0.5 * min(17 ** -0.5, 17 * 4000 ** -1.5)) < 1e-12   # noam.py:19-25
    assert lit["lr_schedulers"][0]["last_epoch"] == 17 and lit["lr_schedulers"][0]["warmup_steps"] == 4000
    back = ck.from_lightning_optimizer_state(cfg, {"optimizer_states": [opt.state_dict()], "lr_schedulers": lit["lr_schedulers"]})
    assert back["step"] == 17
    # the dropout-mask counter must not restart at 0 (it would replay the masks of steps 0..N)
    assert back["micro_step"] == 17
    assert ck.from_lightning_optimizer_state(cfg, {"optimizer_states": [opt.state_dict()], "lr_schedulers": lit["lr_schedulers"]},
                                             accumulate_grad_batches=3)["micro_step"] == 51
    assert ck.from_lightning_optimizer_state(cfg, {"optimizer_states": [opt.state_dict()], "lr_schedulers": lit["lr_schedulers"],
                                                   "fs2_micro_step": 40})["micro_step"] == 40
    assert set(back["exp_avg"]) == set(train)
    for n in train:
        assert torch.equal(back["exp_avg"][n], st["exp_avg"][n]) and torch.equal(back["exp_avg_sq"][n], st["exp_avg_sq"][n])
    # torch 1.10 (what the reference pins) keeps `step` as an int
    old = opt.state_dict()
    for v in old["state"].values():
        v["step"] = int(v["step"])
    assert ck.from_lightning_optimizer_state(cfg, {"optimizer_states": [old], "lr_schedulers": []})["step"] == 17
    wrong = opt.state_dict()
    wrong["param_groups"][0]["params"] = wrong["param_groups"][0]["params"][:-1]
    with pytest.raises(ValueError, match="optimizer holds"):
        ck.from_lightning_optimizer_state(cfg, {"optimizer_states": [wrong]})
