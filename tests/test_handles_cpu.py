"""The host plumbing every handle shares, pinned on the CPU: what `*_load_weight`, `*_finalize`, `*_last_error` and `*_destroy`
answer for the four weight-taking families (engine, HiFi-GAN generator, stochastic duration predictor, FastDiff), and what the
Python `Handle` base does around them.  No device is needed: `*_create` and `*_load_weight` make no HIP call, and `*_finalize`
with a weight missing returns before its first one."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _voc16
from lightningfastspeech2_amd import _lib, fastdiff, hifigan
from lightningfastspeech2_amd.config import Fs2Config
from lightningfastspeech2_amd.weights import SDP_PREFIX, sdp_on_path, state_dict_spec

OK, ARG, WEIGHT = _lib.FS2_OK, _lib.FS2_ERR_ARG, _lib.FS2_ERR_WEIGHT


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _engine(lib):
    cfg = Fs2Config(encoder_layers=2, decoder_layers=2, encoder_kernel_sizes=[5, 9], decoder_kernel_sizes=[9, 3])
    h = C.c_void_p()
    assert lib.fs2_create(C.byref(_lib.config_to_c(cfg, _lib.FS2_F32)), C.byref(h)) == OK, lib.fs2_last_error(h)
    return h, {k: tuple(v) for k, v in state_dict_spec(cfg).items()}


def _vocoder(lib):
    cfg = _voc16.two_stage_cfg()
    h = C.c_void_p()
    assert lib.fs2_voc_create(C.byref(hifigan._config_to_c(cfg, _lib.FS2_BF16)), C.byref(h)) == OK
    return h, {k: tuple(v) for k, v in hifigan.state_dict_spec(cfg).items()}


def _sdp(lib):
    cfg = Fs2Config(n_phones=20, encoder_layers=1, decoder_layers=1, encoder_kernel_sizes=[3], decoder_kernel_sizes=[3], variances=[],
                    variance_levels=[], variance_transforms=[], variance_nlayers=[], variance_kernel_size=[], duration_nlayers=2,
                    duration_kernel_size=3, duration_filter_size=256, duration_depthwise_conv=False, duration_stochastic=True)
    h = C.c_void_p()
    assert lib.fs2_sdp_create(_lib.FS2_ABI_VERSION, 256, 256, 3, 2, C.byref(h)) == OK, lib.fs2_sdp_last_error(h)
    return h, {k[len(SDP_PREFIX):]: tuple(s) for k, s in state_dict_spec(cfg).items() if k.startswith(SDP_PREFIX)}


def _fastdiff(lib):
    cfg = fastdiff.FastDiffConfig()
    ratios = (C.c_int32 * len(cfg.upsample_ratios))(*cfg.upsample_ratios)
    h = C.c_void_p()
    assert lib.fs2_fd_create(_lib.FS2_ABI_VERSION, _lib.FS2_F32, *cfg._c_args(ratios), C.byref(h)) == OK, lib.fs2_fd_last_error(h)
    return h, {k: tuple(v) for k, v in fastdiff.state_dict_spec(cfg).items()}


# prefix of the family's entry points, its create, the text of *_last_error(NULL), which expected names finalize insists on
FAMILIES = {"engine": ("fs2", _engine, b"null engine", lambda n: True),
            "vocoder": ("fs2_voc", _vocoder, b"null vocoder", lambda n: True),
            "sdp": ("fs2_sdp", _sdp, b"null sdp handle", sdp_on_path),
            "fastdiff": ("fs2_fd", _fastdiff, b"null fastdiff handle", lambda n: True)}


class Family:
    def __init__(self, lib, key):
        self.lib = lib
        self.prefix, self.create, self.null_text, self.required = FAMILIES[key]

    def fn(self, what):
        return getattr(self.lib, f"{self.prefix}_{what}")

    def load(self, h, name, shape):
        a = np.zeros(shape, np.float32)
        return self.fn("load_weight")(h, name.encode(), a.ctypes.data_as(C.c_void_p), (C.c_int64 * len(shape))(*shape), len(shape))

    def error(self, h):
        return self.fn("last_error")(h).decode()


@pytest.fixture(params=sorted(FAMILIES))
def fam(request, lib):
    return Family(lib, request.param)


def test_load_weight_checks_name_shape_and_pointers(fam):
    h, spec = fam.create(fam.lib)
    try:
        name, shape = next((n, s) for n, s in spec.items() if len(s) >= 2)
        assert fam.load(h, "no.such.tensor", (4,)) == WEIGHT and "no.such.tensor" in fam.error(h)
        assert fam.load(h, name, shape[:-1] + (shape[-1] + 1,)) == WEIGHT and "shape mismatch" in fam.error(h)  # a wrong dimension
        assert fam.load(h, name, shape[:-1]) == WEIGHT and "shape mismatch" in fam.error(h)                     # a wrong rank
        assert fam.load(h, name, shape + (1,)) == WEIGHT and "shape mismatch" in fam.error(h)
        a = np.zeros(shape, np.float32)
        data, shp = a.ctypes.data_as(C.c_void_p), (C.c_int64 * len(shape))(*shape)
        assert fam.fn("load_weight")(h, None, data, shp, len(shape)) == ARG
        assert fam.fn("load_weight")(h, name.encode(), None, shp, len(shape)) == ARG
        assert fam.fn("load_weight")(h, name.encode(), data, None, len(shape)) == ARG
        assert fam.fn("load_weight")(None, name.encode(), data, shp, len(shape)) == ARG
        assert fam.load(h, name, shape) == OK
        assert fam.load(h, name, shape) == OK  # a second load of the same name overwrites
    finally:
        fam.fn("destroy")(h)


@pytest.mark.parametrize("which", ["first", "last"])
def test_finalize_names_the_one_missing_weight(fam, which):
    h, spec = fam.create(fam.lib)
    try:
        needed = [n for n in spec if fam.required(n)]
        withheld = needed[0] if which == "first" else needed[-1]
        for name, shape in spec.items():
            if name != withheld:
                assert fam.load(h, name, shape) == OK, (name, fam.error(h))
        assert fam.fn("finalize")(h) == WEIGHT
        assert "missing weight" in fam.error(h) and f"'{withheld}'" in fam.error(h)
    finally:
        assert fam.fn("destroy")(h) in (OK, None)  # the half-loaded handle goes away cleanly (fs2_voc_destroy returns void)


def test_last_error_of_a_null_handle(fam, lib):
    assert fam.fn("last_error")(None) == fam.null_text
    assert lib.fs2_mel_last_error(None) == b"null mel handle"


def test_sdp_training_only_tensors_are_checked_and_not_required(lib):
    fam = Family(lib, "sdp")
    h, spec = fam.create(lib)
    try:
        assert spec["sdp.post_pre.weight"] == (256, 1, 1) and not sdp_on_path("sdp.post_pre.weight")
        assert fam.load(h, "sdp.post_pre.weight", (256, 1, 1)) == OK
        assert fam.load(h, "sdp.post_pre.weight", (256, 1)) == WEIGHT and "shape mismatch" in fam.error(h)
        assert fam.load(h, "sdp.post_pre.weight", (128, 1, 1)) == WEIGHT and "shape mismatch" in fam.error(h)
    finally:
        lib.fs2_sdp_destroy(h)
    # every inference tensor but one, no training-only tensor at all: finalize names that one, never a training-only tensor
    h, spec = fam.create(lib)
    try:
        for name, shape in spec.items():
            if sdp_on_path(name) and name != "sdp.proj.bias":
                assert fam.load(h, name, shape) == OK, name
        assert lib.fs2_sdp_finalize(h) == WEIGHT and "missing weight 'sdp.proj.bias'" in fam.error(h)
    finally:
        lib.fs2_sdp_destroy(h)


# ---- the Python base: a fake library, no device
class _FakeLib:
    """fs2_t_* entry points made of plain callables; records every call by name."""

    def __init__(self, finalize_status=0, load_status=0):
        self.calls = []
        self.loaded = {}

        def load_weight(h, name, data, shape, ndim):
            self.calls.append("load_weight")
            self.loaded[name.decode()] = tuple(shape[i] for i in range(ndim))
            return load_status

        def rec(name, result):
            def f(*a):
                self.calls.append(name)
                return result
            return f
        ns = SimpleNamespace(fs2_t_load_weight=load_weight, fs2_t_finalize=rec("finalize", finalize_status),
                             fs2_t_destroy=rec("destroy", None), fs2_t_last_error=lambda h: b"the family's message",
                             fs2_status_string=lambda s: b"status text")
        self.__dict__.update(ns.__dict__)


def _fake_handle_class():
    class T(_lib.Handle):
        _prefix = "fs2_t"

        def __init__(self, lib, weights):
            _lib.Handle.__init__(self, lib)
            self.handle = C.c_void_p(1234)  # what a *_create call leaves
            try:
                self.load_weights(list(weights), weights)
            except Exception:
                self.close()
                raise
    return T


def test_python_handle_loads_checks_and_closes():
    T = _fake_handle_class()
    fake = _FakeLib()
    t = T(fake, {"a.weight": np.zeros((2, 3), np.float64), "b.bias": np.zeros((3,), np.float32)})
    assert fake.calls == ["load_weight", "load_weight", "finalize"] and fake.loaded == {"a.weight": (2, 3), "b.bias": (3,)}
    with pytest.raises(RuntimeError, match="the family's message"):
        t._check(_lib.FS2_ERR_STATE, "anything")
    t._check(_lib.FS2_OK, "anything")
    t.close()
    t.close()  # idempotent
    assert fake.calls.count("destroy") == 1 and not t.handle
    del t
    assert fake.calls.count("destroy") == 1


@pytest.mark.parametrize("failing", ["finalize", "load_weight"])
def test_python_handle_destroys_once_when_the_constructor_fails(failing):
    T = _fake_handle_class()
    fake = _FakeLib(**{f"{'finalize' if failing == 'finalize' else 'load'}_status": _lib.FS2_ERR_WEIGHT})
    with pytest.raises(RuntimeError, match="the family's message"):
        T(fake, {"a.weight": np.zeros((2, 3), np.float32)})
    assert fake.calls.count("destroy") == 1 and fake.calls[-1] == "destroy"


@pytest.mark.parametrize("cls, prefix", [("model.Engine", "fs2"), ("hifigan.HifiGan", "fs2_voc"), ("fastdiff.FastDiff", "fs2_fd"),
                                         ("sdp.StochasticDurationPredictor", "fs2_sdp"), ("analysis.MelAnalyzer", "fs2_mel")])
def test_every_wrapper_derives_from_the_handle_base(lib, cls, prefix):
    import importlib
    mod, name = cls.split(".")
    k = getattr(importlib.import_module(f"lightningfastspeech2_amd.{mod}"), name)
    assert issubclass(k, _lib.Handle) and k._prefix == prefix and k.close is _lib.Handle.close
    for what in ("last_error", "destroy"):
        assert hasattr(lib, f"{prefix}_{what}")
