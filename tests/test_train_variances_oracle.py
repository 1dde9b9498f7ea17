"""CPU: the level- and CWT-aware training helper (tests/_train_variances.py: autograd over the forward oracle + the
reference's loss restated for phone-level and CWT variances) against the three fixtures the REAL reference produced
(tools/gen_golden_train_variances.py), and checkpoint.parameter_order against the reference's own named_parameters() order.
Tolerances are the project's: losses 1e-5 relative, gradients 1e-4 of each tensor's largest entry."""
import pytest

from _train_variances import CASES, VarianceOracleTrainer, check_grads, load_fixture
from lightningfastspeech2_amd import checkpoint

GRAD_TOL = 1e-4


@pytest.mark.parametrize("name", CASES)
def test_helper_reproduces_the_reference_fixture(name):
    z, cfg, sd, batch, hyper = load_fixture(name)
    tr = VarianceOracleTrainer(cfg, sd, **hyper)
    ls, _ = tr.training_step(batch)
    assert list(ls) == [k[5:] for k in z.files if k.startswith("loss_")]
    for k, v in ls.items():
        w = float(z[f"loss_{k}"])
        assert abs(v - w) <= 1e-5 * max(1.0, abs(w)), (k, v, w)
    check_grads(tr.gradients(), {k[5:]: z[k] for k in z.files if k.startswith("grad_")}, GRAD_TOL)


@pytest.mark.parametrize("name", CASES)
def test_parameter_order_is_the_reference_models(name):
    z, cfg, _, _, _ = load_fixture(name)
    assert checkpoint.parameter_order(cfg) == [str(n) for n in z["param_order"]]


def test_fixture_files_stay_small():
    import os
    from _train_variances import GOLD_DIR
    for f in os.listdir(GOLD_DIR):
        if f.startswith(tuple(CASES)):
            assert os.path.getsize(os.path.join(GOLD_DIR, f)) < 1 << 20, f


def test_lightning_optimizer_state_places_the_cwt_head():
    """AdamW's numbering follows the reference's parameters(): the (10, filter) head and mean_std_linear.* land in the slots the
    fixture's param_order gives them, through to_ / from_lightning_optimizer_state and back"""
    import torch
    from lightningfastspeech2_amd.weights import state_dict_spec
    z, cfg, _, _, _ = load_fixture("train_classdefault_small")
    order = [str(n) for n in z["param_order"]]
    spec = state_dict_spec(cfg)
    names = [n for n in order if not n.endswith(".bins")]
    st = {"step": 3, "exp_avg": {n: torch.full(tuple(spec[n]), float(i)) for i, n in enumerate(names)},
          "exp_avg_sq": {n: torch.full(tuple(spec[n]), 0.5 * i) for i, n in enumerate(names)}}
    ck = checkpoint.to_lightning_optimizer_state(cfg, st, lr=2e-3, warmup_steps=4)
    state = ck["optimizer_states"][0]["state"]
    for n in ("variance_adaptor.encoders.pitch.predictor.linear.weight", "variance_adaptor.encoders.pitch.mean_std_linear.weight",
              "variance_adaptor.encoders.pitch.mean_std_linear.bias"):
        assert tuple(state[order.index(n)]["exp_avg"].shape) == tuple(spec[n])
        assert float(state[order.index(n)]["exp_avg"].flatten()[0]) == float(names.index(n))
    assert tuple(spec["variance_adaptor.encoders.pitch.predictor.linear.weight"]) == (10, cfg.variance_filter_size)
    back = checkpoint.from_lightning_optimizer_state(cfg, ck)
    assert back["step"] == 3 and all(torch.equal(back["exp_avg"][n], st["exp_avg"][n]) for n in names)


def test_cwt_head_operators_check_their_arguments_on_the_host():
    """the width / pointer checks run before any launch: no device needed"""
    from lightningfastspeech2_amd import _lib
    lib = _lib.load()
    assert lib.fs2_op_cwt_head_train_ws_bytes(32, 1536, 256) == 32 * 24 * 256 * 4  # one partial per 64 rows of an utterance
    assert lib.fs2_op_cwt_head_bwd_ws_bytes(32, 1536, 256) >= 32 * 24 * (10 * 256 + 10) * 4
    for F in (100, 32, 1088):
        assert lib.fs2_op_cwt_head_train(_lib.FS2_F32, *[None] * 10, 2, 5, F, None) == _lib.FS2_ERR_ARG
        assert lib.fs2_op_cwt_head_bwd(_lib.FS2_F32, *[None] * 12, 2, 5, F, None) == _lib.FS2_ERR_ARG
    assert lib.fs2_op_cwt_head_train(_lib.FS2_F32, *[None] * 10, 2, 5, 128, None) == _lib.FS2_ERR_ARG  # null tensors
