"""CPU-side checks of precision="mixed16" (FS2_MIXED_F16_X3) and the FS2_F16 storage type: the constants and the Python gate, engine
creation and workspace sizes (no device: the layout run on a counting arena), and the host fp32 -> binary16 conversion that
fs2_finalize converts the decoder's weights with, bit for bit against the rule include/fs2.h states."""
import ctypes as C
import os

import pytest
import torch

import _f16
from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.config import preset
from lightningfastspeech2_amd.weights import synth_state_dict


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _create(lib, cfg, dtype):
    cc = _lib.config_to_c(cfg, dtype)
    h = C.c_void_p()
    return lib.fs2_create(C.byref(cc), C.byref(h)), h


def test_constants_and_python_gate():
    assert _lib.FS2_F16 == 5 and _lib.FS2_MIXED_F16_X3 == 6
    from lightningfastspeech2_amd import model
    assert model._PRECISIONS["mixed16"] == _lib.FS2_MIXED_F16_X3
    assert model._PRECISIONS["mixed3"] == _lib.FS2_MIXED_X3  # (nothing moved)
    from lightningfastspeech2_amd.training import Trainer
    cfg = preset("c2")
    with pytest.raises(ValueError, match="precision must be one of"):
        Trainer(cfg, synth_state_dict(cfg, 1), precision="mixed16")


@pytest.mark.parametrize("name", ["c2", "c3", "ref-default"])
def test_create_and_workspace_equal_mixed3(lib, name):
    """The element sizes of "mixed16" are "mixed3"'s (fp32 front, 2-byte back): so is every workspace size."""
    assert lib.fs2_abi_version() == 4
    cfg = preset(name)
    st16, h16 = _create(lib, cfg, _lib.FS2_MIXED_F16_X3)
    st3, h3 = _create(lib, cfg, _lib.FS2_MIXED_X3)
    try:
        assert st16 == 0, lib.fs2_last_error(h16)
        assert st3 == 0
        for B in (1, 4):
            for L in (1, 64, 65):
                for T in (0, 1, 65, 300):
                    a, b = (C.c_size_t(), C.c_size_t()), (C.c_size_t(), C.c_size_t())
                    assert lib.fs2_workspace_bytes(h16, B, L, T, C.byref(a[0]), C.byref(a[1])) == 0
                    assert lib.fs2_workspace_bytes(h3, B, L, T, C.byref(b[0]), C.byref(b[1])) == 0
                    assert (a[0].value, a[1].value) == (b[0].value, b[1].value) and a[0].value > 0, (B, L, T)
    finally:
        lib.fs2_destroy(h16)
        lib.fs2_destroy(h3)


def test_f16_alone_is_not_an_engine_mode(lib):
    st, h = _create(lib, preset("c2"), _lib.FS2_F16)
    assert st == 3  # FS2_ERR_ARG: a storage dtype of the operators
    lib.fs2_destroy(h)


def test_host_conversion_saturates_and_rounds_to_nearest_even(lib):
    x = _f16.edge_values()
    got = torch.empty(x.numel(), dtype=torch.int16)
    assert lib.fs2_host_f32_to_f16(x, got, x.numel()) == 0
    want = _f16.f16_bits(x)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, [(float(x[i]), hex(int(got[i]) & 0xFFFF), hex(int(want[i]) & 0xFFFF)) for i in bad[:8]]
    back = got.view(torch.float16).float()
    assert float(back[torch.isinf(x) & (x > 0)].max()) == 65504.0 and float(back[torch.isinf(x) & (x < 0)].min()) == -65504.0
    assert bool(torch.isnan(back[torch.isnan(x)]).all()) and bool(torch.isfinite(back[~torch.isnan(x)]).all())
