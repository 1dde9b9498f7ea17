"""The stochastic duration predictor without a GPU: the CPU restatement tests/_sdp_ref.py against the reference's fixtures
(tests/golden/sdp, tools/gen_golden_sdp.py) and, where the reference is present, against its live modules; what fs2_sdp_* refuses
on the host alone; the config field, the weight names and the checkpoint path."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _sdp_ref as R
from _golden import Golden
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd import checkpoint as ck
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.weights import SDP_PREFIX, sdp_on_path, state_dict_spec, synth_state_dict
from tools.ref_import import reference_available

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdp")
needs_reference = pytest.mark.skipif(not reference_available(), reason="the reference checkout is not on this machine")


def _live_wrapper(n, hidden):
    """The reference's own StochasticDurationPredictorWrapper(nlayers, in_channels, filter_size, kernel_size, dropout)
    (model.py:463-473).  Importing the reference installs stand-ins for packages this machine lacks (tools/ref_import.py); other
    tests look at sys.modules, so every module this import added is taken out again - the class itself stays usable."""
    import sys
    from tools import ref_import
    before = set(sys.modules)
    try:
        m, _ = ref_import.load_reference()
        wrapper = m.StochasticDurationPredictorWrapper(n, hidden, 256, 3, 0.5)
    finally:
        for k in set(sys.modules) - before:  # the reference and the stand-ins; real packages it pulled in may stay
            if k.split(".")[0] in ("litfass", "pytorch_lightning", "torchaudio", "wandb", "pysdtw", "numba"):
                del sys.modules[k]
        ref_import._loaded = None
    return wrapper.eval()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _module_fixture(n):
    z = np.load(os.path.join(GOLDEN, f"module_n{n}.npz"))
    cfg = Fs2Config.from_json(str(z["config_json"]))
    rc = json.loads(str(z["recipe_json"]))
    w = R.sdp_state_dict(cfg, rc["weights_seed"])
    x, pad = R.module_inputs(rc["inputs_seed"])
    assert R.digest(w, x, pad) == str(z["sha256"]), "the synthetic recipe drifted from the fixture"
    return cfg, w, x, pad, z


# ---- the restatement against the reference's outputs
@pytest.mark.parametrize("n", [1, 2, 3])
def test_ref_float64_equals_the_reference_float64(n):
    cfg, w, x, pad, z = _module_fixture(n)
    assert cfg.duration_stochastic and cfg.duration_nlayers == n
    logw = R.sdp_logw(R.sdp_weights(w, torch.float64), x, pad, z["noise"]).numpy()
    assert np.abs(logw - z["logw64"]).max() <= 1e-9  # float64 on both sides: only the order of the sums differs
    assert (logw[pad] == 0).all()
    d, guard = R.durations_stochastic(logw, pad)
    assert not guard.any() and np.array_equal(d.numpy(), z["durations"])
    # the fixture keeps what it promises: no exp(logw64) within 5e-5 relative of an integer
    e = np.exp(z["logw64"][~pad])
    assert (np.abs(e - np.rint(e)) > 5e-5 * e).all()


def test_ref_spline_equals_the_reference_float64():
    z = np.load(os.path.join(GOLDEN, "spline.npz"))
    x1, h = torch.as_tensor(z["x1"]).double(), torch.as_tensor(z["h29"]).double()
    out, disc, bins = R.spline_inverse(x1, h, 16.0, return_details=True)
    assert np.abs(out.numpy() - z["out64"]).max() <= 1e-9
    assert float(disc.min()) >= 1e-6
    assert sorted(set(bins[bins >= 0].tolist())) == list(range(10))  # every one of the spline's own ten bins is visited
    x = z["x1"]
    five = np.float32(5.0)
    for v in (five, -five, np.nextafter(five, np.float32(0)), np.nextafter(five, np.float32(10))):  # the bound and a step to each side
        assert (x == v).any() and (x == -v).any()
    assert (x > 6).any() and (x < -6).any()
    inside = np.abs(z["out64"]) < 5
    assert len(np.unique(np.floor(z["out64"][inside]).astype(int))) == 10  # every unit interval of the output range is hit
    outside = np.abs(x) > 5
    assert np.array_equal(z["out64"][outside], x[outside].astype(np.float64))


def test_durations_rule():
    logw = np.array([[0.0, np.log(2.5), np.log(3.0) + 1e-3, -4.0, 0.0]], np.float32)
    d, guard = R.durations_stochastic(logw)
    assert d.tolist() == [[0, 3, 4, 1, 0]] and not guard.any()
    d, guard = R.durations_stochastic(np.zeros((1, 4), np.float32), np.array([[False, False, False, True]]))
    assert d.tolist() == [[1, 1, 1, 0]] and guard.all()  # 0 <= 3 // 2: the zero-duration guard


# ---- against the live reference
@needs_reference
@pytest.mark.parametrize("n", [1, 2, 4])
def test_spec_equals_the_reference_wrapper(n):
    cfg = R.module_config(n, hidden=64)
    own = {k: tuple(v.shape) for k, v in _live_wrapper(n, 64).state_dict().items()}
    spec = {k[len(SDP_PREFIX):]: tuple(s) for k, s in state_dict_spec(cfg).items() if k.startswith(SDP_PREFIX)}
    assert list(spec.items()) == list(own.items())  # names, shapes and order
    dropped = [k for k in spec if not sdp_on_path(k)]
    assert all(k.startswith(("sdp.post_", "sdp.flows.1.")) for k in dropped) and len(dropped) > len(spec) // 2


@needs_reference
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_ref_matches_the_live_module(seed):
    n = 1 + seed % 3
    cfg = R.module_config(n, hidden=64)
    w = R.sdp_state_dict(cfg, seed)
    mod = _live_wrapper(n, 64)
    mod.load_state_dict({k: torch.as_tensor(v) for k, v in w.items()}, strict=True)
    mod = mod.double()
    x, pad = R.module_inputs(seed + 1, B=2, L=40, lengths=(40, 17), hidden=64)
    torch.manual_seed(seed)
    noise = torch.randn(2, 2, 40)
    torch.manual_seed(seed)
    with torch.no_grad():
        want = mod(torch.as_tensor(x).double(), torch.as_tensor(pad), inference=True).numpy()
    got = R.sdp_logw(R.sdp_weights(w, torch.float64), x, pad, noise).numpy()
    assert np.abs(got - want).max() <= 1e-9


# ---- host-side validation of the handle
def _create(lib, H=256, F=256, k=3, n=2, abi=None):
    h = C.c_void_p()
    st = lib.fs2_sdp_create(_lib.FS2_ABI_VERSION if abi is None else abi, H, F, k, n, C.byref(h))
    return st, h


def _load(lib, h, name, shape):
    a = np.zeros(shape, np.float32)
    return lib.fs2_sdp_load_weight(h, name.encode(), a.ctypes.data_as(C.c_void_p), (C.c_int64 * len(shape))(*shape), len(shape))


def test_create_refuses_on_the_host(lib):
    ARG, SHAPE = _lib.FS2_ERR_ARG, _lib.FS2_ERR_SHAPE
    for kw, code, text in ((dict(abi=3), ARG, "abi_version"), (dict(F=128), SHAPE, "256 channels"), (dict(k=5), SHAPE, "k = 3"),
                           (dict(n=0), SHAPE, "n_flows"), (dict(n=9), SHAPE, "n_flows"), (dict(H=264), SHAPE, "in_channels"),
                           (dict(H=24), SHAPE, "in_channels")):
        st, h = _create(lib, **kw)
        assert st == code and h.value and text in lib.fs2_sdp_last_error(h).decode(), kw
        assert lib.fs2_sdp_tile_rows(h) == 0 and _load(lib, h, "sdp.pre.bias", (256,)) == _lib.FS2_ERR_STATE
        assert lib.fs2_sdp_destroy(h) == 0
        args = dict(H=256, F=256, k=3, n=2)
        args.update({k: v for k, v in kw.items() if k != "abi"})
        if "abi" not in kw:
            assert lib.fs2_sdp_supported(args["H"], args["F"], args["k"], args["n"]) == 0
    assert lib.fs2_sdp_supported(256, 256, 3, 2) == 1 and lib.fs2_sdp_supported(64, 256, 3, 8) == 1
    assert lib.fs2_sdp_create(_lib.FS2_ABI_VERSION, 256, 256, 3, 2, None) == ARG
    assert lib.fs2_sdp_destroy(None) == ARG and lib.fs2_sdp_last_error(None) == b"null sdp handle"


def test_load_weight_and_finalize_validation(lib):
    WEIGHT = _lib.FS2_ERR_WEIGHT
    st, h = _create(lib, H=64, n=3)
    assert st == 0 and lib.fs2_sdp_tile_rows(h) > 26 and lib.fs2_sdp_launches(h) == 3
    try:
        assert _load(lib, h, "sdp.nonsense.weight", (256,)) == WEIGHT and b"unknown weight name" in lib.fs2_sdp_last_error(h)
        assert _load(lib, h, "sdp.flows.4.pre.weight", (256, 1, 1)) == WEIGHT  # a flow this predictor does not have
        assert _load(lib, h, "sdp.pre.weight", (256, 256, 1)) == WEIGHT and b"shape mismatch" in lib.fs2_sdp_last_error(h)
        assert _load(lib, h, "sdp.pre.weight", (256, 64)) == WEIGHT
        assert _load(lib, h, "sdp.pre.weight", (256, 64, 1)) == 0
        for name, shape in (("sdp.post_pre.weight", (256, 1, 1)), ("sdp.post_flows.2.proj.weight", (29, 256, 1)),
                            ("sdp.flows.1.convs.norms_1.0.gamma", (256,)), ("sdp.post_flows.0.log_scale", (2, 1))):
            assert _load(lib, h, name, shape) == 0, name              # training-only: accepted (and dropped)
        assert _load(lib, h, "sdp.post_pre.weight", (256, 1)) == WEIGHT  # ... but still shape-checked
        assert lib.fs2_sdp_finalize(h) == WEIGHT and b"missing weight" in lib.fs2_sdp_last_error(h)
        n = C.c_size_t()
        assert lib.fs2_sdp_workspace_bytes(h, 2, 30, C.byref(n)) == 0 and n.value >= 2 * 30 * 256 * 4 + 2 * 2 * 2 * 30 * 4
        assert lib.fs2_sdp_workspace_bytes(h, 0, 30, C.byref(n)) == _lib.FS2_ERR_ARG
        assert lib.fs2_sdp_forward(h, _lib.FS2_F32, None, None, None, None, None, 0, 1, 1, None) == _lib.FS2_ERR_STATE  # not finalized
    finally:
        lib.fs2_sdp_destroy(h)


def test_every_on_path_tensor_is_required_and_no_other(lib):
    """finalize names a missing tensor exactly when it is on the inference path: load everything but one, for every name"""
    cfg = R.module_config(2, hidden=64)
    spec = {k[len(SDP_PREFIX):]: s for k, s in state_dict_spec(cfg).items() if k.startswith(SDP_PREFIX)}
    for skip in list(spec)[::7]:
        st, h = _create(lib, H=64, n=2)
        try:
            for name, shape in spec.items():
                if name != skip:
                    assert _load(lib, h, name, shape) == 0, name
            if sdp_on_path(skip):
                assert lib.fs2_sdp_finalize(h) == _lib.FS2_ERR_WEIGHT and skip.encode() in lib.fs2_sdp_last_error(h), skip
            # (a complete on-path set goes on to the device upload: tests/test_gpu_sdp.py)
        finally:
            lib.fs2_sdp_destroy(h)


def test_engine_switch_is_validated_on_the_host(lib):
    """fs2_set_stochastic_duration: refused with a depth-wise duration predictor, after a weight, and for an unsupported shape;
    the engine then takes the sdp.* names and refuses the deterministic predictor's"""
    def engine(**kw):
        cfg = Fs2Config(n_phones=20, encoder_hidden=64, decoder_hidden=64, encoder_layers=1, decoder_layers=1,
                        encoder_kernel_sizes=[3], decoder_kernel_sizes=[3], encoder_conv_filter_size=64, decoder_conv_filter_size=64,
                        encoder_depthwise_conv=False, decoder_depthwise_conv=False, variance_filter_size=64,
                        variance_depthwise_conv=False, duration_nlayers=1, **kw)
        h = C.c_void_p()
        assert lib.fs2_create(C.byref(_lib.config_to_c(cfg, _lib.FS2_F32)), C.byref(h)) == 0, lib.fs2_last_error(h)
        return h
    z = np.zeros(256 * 64, np.float32)

    def load(h, name, shape):
        return lib.fs2_load_weight(h, name.encode(), z.ctypes.data_as(C.c_void_p), (C.c_int64 * len(shape))(*shape), len(shape))
    h = engine(duration_filter_size=256, duration_depthwise_conv=True)
    assert lib.fs2_set_stochastic_duration(h, 1) == _lib.FS2_ERR_SHAPE and b"depthwise" in lib.fs2_last_error(h)
    lib.fs2_destroy(h)
    h = engine(duration_filter_size=128, duration_depthwise_conv=False)
    assert lib.fs2_set_stochastic_duration(h, 1) == _lib.FS2_ERR_SHAPE and b"256 channels" in lib.fs2_last_error(h)
    lib.fs2_destroy(h)
    h = engine(duration_filter_size=256, duration_depthwise_conv=False)
    dur = "variance_adaptor.duration_predictor."
    assert lib.fs2_set_duration_noise(h, C.c_void_p(256), 1, 4) == _lib.FS2_ERR_STATE  # not a stochastic engine (yet)
    assert lib.fs2_set_stochastic_duration(h, 1) == 0
    assert load(h, dur + "layers.0.layers.0.module.weight", (256, 64, 3)) == _lib.FS2_ERR_WEIGHT
    assert load(h, dur + "sdp.pre.weight", (256, 64, 1)) == 0
    assert load(h, dur + "sdp.post_pre.bias", (256,)) == 0
    assert load(h, dur + "sdp.flows.2.pre.bias", (256,)) == _lib.FS2_ERR_WEIGHT  # duration_nlayers = 1: one flow
    assert lib.fs2_set_stochastic_duration(h, 0) == _lib.FS2_ERR_STATE             # a weight has been loaded
    lib.fs2_destroy(h)
    h = engine(duration_filter_size=256, duration_depthwise_conv=False)
    assert lib.fs2_set_stochastic_duration(h, 1) == 0 and lib.fs2_set_stochastic_duration(h, 0) == 0  # off again: the old names
    assert load(h, dur + "layers.0.layers.0.module.weight", (256, 64, 3)) == 0
    assert load(h, dur + "sdp.pre.weight", (256, 64, 1)) == _lib.FS2_ERR_WEIGHT
    lib.fs2_destroy(h)


def test_engine_takes_a_narrow_model_with_the_default_two_flows(lib):
    """hidden 64, duration_filter_size 256, duration_nlayers 2 (the class default): the conv predictor's filter == hidden rule does
    not concern the flow predictor - fs2_create accepts the config, the switch turns it stochastic and the engine takes every sdp.*
    name of the spec; WITHOUT the switch the first weight is refused with the conv predictor's message."""
    cfg = R.module_config(2, hidden=64)
    spec = {k: s for k, s in state_dict_spec(cfg).items() if k.startswith(SDP_PREFIX)}
    z = np.zeros(256 * 256, np.float32)

    def load(h, name, shape):
        return lib.fs2_load_weight(h, name.encode(), z.ctypes.data_as(C.c_void_p), (C.c_int64 * len(shape))(*shape), len(shape))
    h = C.c_void_p()
    assert lib.fs2_create(C.byref(_lib.config_to_c(cfg, _lib.FS2_F32)), C.byref(h)) == 0, lib.fs2_last_error(h)
    assert lib.fs2_set_stochastic_duration(h, 1) == 0, lib.fs2_last_error(h)
    for name, shape in spec.items():
        assert load(h, name, shape) == 0, (name, lib.fs2_last_error(h))
    assert load(h, "linear.bias", (cfg.n_mels,)) == 0  # and the rest of the model as before
    assert lib.fs2_finalize(h) == _lib.FS2_ERR_WEIGHT and b"missing weight" in lib.fs2_last_error(h)  # (the rest is not loaded here)
    lib.fs2_destroy(h)
    h = C.c_void_p()
    assert lib.fs2_create(C.byref(_lib.config_to_c(cfg, _lib.FS2_F32)), C.byref(h)) == 0
    assert load(h, "linear.bias", (cfg.n_mels,)) == _lib.FS2_ERR_SHAPE and b"duration_filter_size != hidden" in lib.fs2_last_error(h)
    assert lib.fs2_finalize(h) == _lib.FS2_ERR_SHAPE
    lib.fs2_destroy(h)


# ---- config, weights, checkpoint
def test_config_round_trip_and_validation():
    cfg = Fs2Config(duration_stochastic=True, duration_depthwise_conv=False)
    assert cfg.to_dict()["duration_stochastic"] is True
    assert Fs2Config.from_dict(cfg.to_dict()).duration_stochastic and Fs2Config.from_json(cfg.to_json()) == cfg
    assert Fs2Config().duration_stochastic is False and Fs2Config.from_dict({}).duration_stochastic is False
    with pytest.raises(ValueError, match="duration_depthwise_conv"):
        Fs2Config(duration_stochastic=True)  # the class default is depth-wise: refused, as the reference refuses it
    for bad in (dict(duration_filter_size=128), dict(duration_kernel_size=5), dict(duration_nlayers=9), dict(duration_nlayers=0),
                dict(encoder_hidden=512, decoder_hidden=512, variance_filter_size=512)):  # what fs2_sdp_supported refuses
        with pytest.raises(ValueError, match="duration_stochastic"):
            Fs2Config(**{**dict(duration_stochastic=True, duration_depthwise_conv=False), **bad})
    # the flow predictor maps hidden -> filter itself: no filter == hidden demand for more than one flow
    assert Fs2Config(encoder_hidden=128, decoder_hidden=128, variance_filter_size=128, duration_stochastic=True,
                     duration_depthwise_conv=False, duration_nlayers=3, duration_filter_size=256).duration_nlayers == 3
    hp = {k: v for k, v in cfg.to_dict().items() if k not in ("stats", "n_phones")}
    assert Fs2Config.from_hparams(hp, cfg.stats, 80).duration_stochastic


def test_spec_and_synthetic_weights():
    cfg = R.module_config(3)
    spec = state_dict_spec(cfg)
    det = state_dict_spec(Fs2Config.from_dict({**cfg.to_dict(), "duration_stochastic": False, "duration_filter_size": 256}))
    sdp = [k for k in spec if k.startswith(SDP_PREFIX)]
    assert sdp and all(k.startswith(SDP_PREFIX + "sdp.") for k in sdp)
    assert [k for k in spec if not k.startswith(SDP_PREFIX)] == [k for k in det if not k.startswith(SDP_PREFIX)]
    assert spec[SDP_PREFIX + "sdp.flows.3.proj.weight"] == (29, 256, 1) and SDP_PREFIX + "sdp.flows.4.pre.bias" not in spec
    sd = synth_state_dict(cfg, 5)
    assert list(sd) == list(spec) and all(sd[k].shape == tuple(spec[k]) and sd[k].dtype == np.float32 for k in spec)
    proj = sd[SDP_PREFIX + "sdp.flows.2.proj.weight"]
    assert 0.08 < proj.std() < 0.17 and abs(sd[SDP_PREFIX + "sdp.convs.norms_1.0.gamma"].mean() - 1) < 0.1  # not the zero init
    with pytest.raises(ValueError):
        synth_state_dict(cfg, 5, duration_bias=1.0)


@pytest.mark.parametrize("name", ["dense_small", "dw_small", "recipe_small"])
def test_existing_synthetic_state_dicts_are_unchanged(name):
    g = Golden(name)
    assert not g.cfg.duration_stochastic
    g.state_dict()  # asserts the sha256 the fixture was written with


def test_lightning_checkpoint_with_a_stochastic_predictor(tmp_path):
    from test_checkpoint_cpu import _write_lightning_checkpoint
    cfg = R.module_config(2, hidden=64)
    sd = synth_state_dict(cfg, 3)
    path = tmp_path / "lit_model.ckpt"
    _write_lightning_checkpoint(path, cfg, sd)
    c = ck.read_checkpoint(path)
    cfg2 = ck.config_from_checkpoint(c)
    assert cfg2.duration_stochastic and cfg2.to_dict() == cfg.to_dict()
    w, rep = ck.resolve_state_dict(cfg2, c["state_dict"])
    assert set(w) == set(state_dict_spec(cfg)) and not rep["dropped"]
    np.testing.assert_array_equal(w[SDP_PREFIX + "sdp.post_flows.2.proj.bias"], sd[SDP_PREFIX + "sdp.post_flows.2.proj.bias"])


def test_training_and_loss_keep_rejecting_stochastic_durations():
    from lightningfastspeech2_amd.loss import FastSpeech2Loss
    from lightningfastspeech2_amd.training import Trainer
    with pytest.raises(NotImplementedError):
        FastSpeech2Loss(duration_stochastic=True)
    cfg = R.module_config(2, hidden=64)
    with pytest.raises(NotImplementedError, match="stochastic"):
        Trainer(cfg, synth_state_dict(cfg, 1))
