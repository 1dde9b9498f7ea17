"""CPU-side checks of the C-ABI boundary (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lightningfastspeech2_amd import _lib
from lightningfastspeech2_amd.config import Fs2Config, preset
from lightningfastspeech2_amd.weights import state_dict_spec, synth_state_dict


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_library_exports_every_declared_symbol(lib):
    names = _lib.declared_symbols()
    assert len(names) >= 20 and "fs2_encode" in names and "fs2_decode" in names
    for n in names:
        assert hasattr(lib, n), n
    assert lib.fs2_abi_version() == _lib.FS2_ABI_VERSION


def test_struct_layout_matches_header():
    # sizes follow from include/fs2.h: 8 + (4+32)*2 ints, 1 int, 4*32 chars, 2*4 ints, 2*4 floats, 7 ints, n_priors,
    # FS2_MAX_PRIORS names (ABI v3: the shipped recipe lists five priors, scripts/train.sh:49), var_cwt
    assert _lib.FS2_ABI_VERSION == 4 and _lib.FS2_MAX_PRIORS == 8  # v4: var_level (phone-level variances)
    assert C.sizeof(_lib.Fs2ConfigC) == 4 * (8 + 36 + 36 + 1) + 4 * 32 + 4 * (4 + 4) + 4 * (4 + 4) + 4 * 7 + 4 + 8 * 32 + 4 * 4 + 4 * 4  # ... var_cwt, var_level
    assert C.sizeof(_lib.Fs2OutputsC) == 8 * (5 + 3 * _lib.FS2_MAX_VARIANCES)


def test_every_declaration_is_bound_with_explicit_types(lib):
    """The binding is generated from include/fs2.h: the parsed set is the set a loose scan of the header finds, and every member
    carries an explicit restype and one argtype per parameter."""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    loose = {m.group(1): m.group(2) for m in re.finditer(r"\b(fs2_[a-z0-9_]+)\s*\(([^()]*)\)", text)}
    parsed = _lib.parse_header(_lib.HEADER_PATH).functions
    assert len(loose) >= 124 and sorted(loose) == _lib.declared_symbols() == sorted(parsed)
    for name, params in loose.items():
        fn = getattr(lib, name)
        returns_void = re.search(r"\bvoid\s+%s\s*\(" % name, text) is not None
        assert fn.restype is parsed[name][0] and (fn.restype is None) == returns_void, name
        assert fn.argtypes is not None and len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert lib.fs2_abi_version.restype is C.c_int and lib.fs2_abi_version.argtypes == []
    assert lib.fs2_voc_destroy.restype is None


def test_binding_types_where_a_slip_would_hurt(lib):
    assert lib.fs2_op_masked_loss.argtypes[4] is C.c_int64 and lib.fs2_op_masked_loss_bwd.argtypes[6] is C.c_int64
    assert lib.fs2_op_dropout.argtypes[3:7] == [C.c_size_t, C.c_float, C.c_uint64, C.c_uint64]
    assert C.sizeof(C.c_int64) == C.sizeof(C.c_uint64) == C.sizeof(C.c_size_t) == 8
    assert lib.fs2_op_wav_pack.argtypes[7] is C.c_int64
    assert lib.fs2_graph_replays.restype is C.c_int64 and lib.fs2_op_transpose_weight_tiles.restype is C.c_int64
    sizes = [n for n in _lib.declared_symbols() if n.endswith(("_ws_bytes", "_scratch_bytes"))]
    assert len(sizes) >= 8 and "fs2_op_attention_scratch_bytes" in sizes
    for n in sizes:
        assert getattr(lib, n).restype is C.c_size_t, n
    for n in ("fs2_status_string", "fs2_last_error", "fs2_voc_last_error"):
        assert getattr(lib, n).restype is C.c_char_p, n
    assert lib.fs2_create.argtypes[0] is C.POINTER(_lib.Fs2ConfigC) and lib.fs2_create.argtypes[1] is C.POINTER(C.c_void_p)
    assert lib.fs2_op_bgemm.argtypes[1] is C.POINTER(_lib.BGemmDescC)
    assert lib.fs2_voc_create.argtypes[0] is C.POINTER(_lib.Fs2VocConfigC)


def test_generated_structs_match_the_compiler(tmp_path):
    """sizeof / offsetof of every struct and field of include/fs2.h as the host C compiler lays them out (a stand-alone program)
    against the generated ctypes.Structure classes."""
    structs = _lib.parse_header(_lib.HEADER_PATH).structs
    assert sorted(structs) == ["fs2_bgemm_desc", "fs2_config", "fs2_outputs", "fs2_voc_config"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fs2.h"', 'int main(void) {']
    for name, st in structs.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in st._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    cc = [shutil.which("cc")] if shutil.which("cc") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c"]
    assert os.path.exists(cc[0]), "no host C compiler (cc or hipcc) to check the struct layout with"
    exe = str(tmp_path / "layout")
    subprocess.run(cc + [str(src), "-I", os.path.dirname(_lib.HEADER_PATH), "-o", exe], check=True, capture_output=True, text=True)
    got = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        key, *nums = line.split()
        got[key] = tuple(int(n) for n in nums)
    want = {}
    for name, st in structs.items():
        want[name] = (C.sizeof(st),)
        want.update({f"{name}.{f}": (getattr(st, f).offset, getattr(st, f).size) for f, _ in st._fields_})
    assert len(want) == 4 + 81 and got == want
    for py, c in (("Fs2ConfigC", "fs2_config"), ("Fs2OutputsC", "fs2_outputs"), ("BGemmDescC", "fs2_bgemm_desc"), ("Fs2VocConfigC", "fs2_voc_config")):
        assert [(f, C.sizeof(t)) for f, t in getattr(_lib, py)._fields_] == [(f, C.sizeof(t)) for f, t in structs[c]._fields_]


_MINI = """
#define FS2_N 3
enum fs2_e { FS2_A, FS2_B = 5, FS2_C, FS2_D = FS2_N };
typedef struct fs2_s { int32_t a, b[FS2_N][2]; const float* p; char name[FS2_C]; } fs2_s;
typedef struct fs2_h fs2_h;
int fs2_ok(const fs2_s* s, fs2_h** out, const char* name, uint16_t* dst,
           size_t n);
void fs2_none(void);
"""


def test_parser_reads_header_text():
    h = _lib.parse_header(_MINI)
    assert h.constants == {"FS2_N": 3, "FS2_A": 0, "FS2_B": 5, "FS2_C": 6, "FS2_D": 3}
    s = h.structs["fs2_s"]
    assert [f for f, _ in s._fields_] == ["a", "b", "p", "name"] and C.sizeof(s) == 4 + 24 + 4 + 8 + 6 + 2
    assert s.b.size == 24 and len(s().b) == 3 and len(s().b[0]) == 2 and s.p.size == 8 and s.name.size == 6
    assert h.functions == {"fs2_ok": (C.c_int, [C.POINTER(s), C.POINTER(C.c_void_p), C.c_char_p, C.c_void_p, C.c_size_t]),
                           "fs2_none": (None, [])}


@pytest.mark.parametrize("decl,named", [
    ("int fs2_bad(long n);", "fs2_bad"),                                   # a scalar outside the table
    ("int fs2_bad(unsigned n);", "fs2_bad"),
    ("long fs2_bad(void);", "fs2_bad"),
    ("int fs2_bad(const fs2_undeclared* d);", "fs2_bad"),                  # a pointer to a type the header does not declare
    ("int fs2_bad(const struct fs2_s* d);", "fs2_bad"),
    ("int fs2_bad(const char* fmt, ...);", "fs2_bad"),                     # variadic
    ("int fs2_bad(int32_t v[4]);", "fs2_bad"),                             # array parameter
    ("int fs2_bad(void (*cb)(int32_t));", "fs2_bad"),                      # function pointer
    ("int fs2_first(void)\nint fs2_bad(void);", "fs2_bad"),                # two prototypes run together (a lost semicolon)
    ("FS2_API int fs2_bad(void);", "fs2_bad"),                             # an attribute macro in front
    ("#define FS2_DECL(n) int n(void)\nFS2_DECL(fs2_hidden);\nint fs2_bad(void)\n;", "fs2_hidden"),  # declared through a macro
    ("#define fs2_old(v) fs2_none()", "fs2_old"),                          # a name only the loose scan sees
    ("typedef struct fs2_t { long x; } fs2_t;", "fs2_t"),                  # a field outside the table
    ("typedef struct fs2_t { int32_t x[FS2_NOPE]; } fs2_t;", "FS2_NOPE"),  # an array bound that is no constant
])
def test_parser_refuses_what_it_cannot_type(decl, named):
    with pytest.raises(_lib.Fs2LibraryError, match=named):
        _lib.parse_header(_MINI + decl + "\n")


def test_constants_are_the_abi_promises():
    assert _lib.FS2_ABI_VERSION == 4
    assert (_lib.FS2_OK, _lib.FS2_ERR_HIP, _lib.FS2_ERR_SHAPE, _lib.FS2_ERR_ARG, _lib.FS2_ERR_WEIGHT, _lib.FS2_ERR_STATE,
            _lib.FS2_ERR_NOMEM) == (0, 1, 2, 3, 4, 5, 6)
    assert (_lib.FS2_F32, _lib.FS2_BF16, _lib.FS2_MIXED, _lib.FS2_MIXED_X3, _lib.FS2_F32_X3, _lib.FS2_F16,
            _lib.FS2_MIXED_F16_X3) == (0, 1, 2, 3, 4, 5, 6)
    assert _lib.FS2_K_COUNT == 8 and _lib.K_PREDICTOR == _lib.FS2_K_PREDICTOR == 7 and _lib.K_CONV_GEMM == 0
    assert (_lib.FS2_MAX_LAYERS, _lib.FS2_MAX_VARIANCES, _lib.FS2_NAME_LEN, _lib.FS2_WAV_I16, _lib.FS2_WAV_F32) == (32, 4, 32, 0, 1)
    assert (_lib.FS2_VOC_MAX_STAGES, _lib.FS2_VOC_MAX_KERNELS) == (8, 4)


def _create(lib, cfg, dtype=_lib.FS2_F32):
    cc = _lib.config_to_c(cfg, dtype)
    h = C.c_void_p()
    st = lib.fs2_create(C.byref(cc), C.byref(h))
    return st, h


def test_create_validates_config(lib):
    st, h = _create(lib, preset("c2"), _lib.FS2_BF16)
    assert st == 0
    lib.fs2_destroy(h)
    bad = Fs2Config(encoder_hidden=96, decoder_hidden=96, encoder_conv_filter_size=192,
                    decoder_conv_filter_size=192, variance_filter_size=96, duration_filter_size=96,
                    encoder_head=1, decoder_head=1)
    st, h = _create(lib, bad)
    assert st == 2 and b"multiple of 64" in lib.fs2_last_error(h)  # FS2_ERR_SHAPE, loud and specific
    lib.fs2_destroy(h)
    st, h = _create(lib, Fs2Config(encoder_head=16, decoder_head=16))  # head dim 16 unsupported
    assert st == 2
    lib.fs2_destroy(h)


def _workspace_configs():
    cwt_stats = {"pitch": {"min": 0.2, "max": 5.0, "mean": 0.1, "std": 1.5}, "energy": {"min": 0.3, "max": 4.0, "mean": 0.0, "std": 1.0},
                 "snr": {"min": -1.0, "max": 4.0, "mean": 1.2, "std": 2.0}}
    phone_cwt2 = Fs2Config(**{**preset("c2").to_dict(), "variance_levels": ["phone", "phone", "frame"],
                              "variance_transforms": ["cwt", "cwt", "none"], "stats": cwt_stats})
    return [("c2-bf16", preset("c2"), _lib.FS2_BF16), ("c3-bf16", preset("c3"), _lib.FS2_BF16),
            ("ref-default-fp32", preset("ref-default"), _lib.FS2_F32), ("c2-phone-cwt2-bf16", phone_cwt2, _lib.FS2_BF16)]


def test_workspace_bytes_grow_with_the_shape(lib):
    """Callers size their two buffers once, for their largest (B, L, T), and run every smaller shape in them: so both sizes
    fs2_workspace_bytes reports must be non-decreasing in each of B, L and T, and persist (the encode phase's state) must not
    depend on T.  No device needed: the sizes are the workspace layout run on an arena that only counts."""
    Bs, Ls, Ts = (1, 4), (1, 63, 64, 65), (0, 1, 64, 65, 300)
    for name, cfg, dtype in _workspace_configs():
        st, h = _create(lib, cfg, dtype)
        assert st == 0, lib.fs2_last_error(h)
        size = {}
        for B in Bs:
            for L in Ls:
                for T in Ts:
                    p, s = C.c_size_t(), C.c_size_t()
                    assert lib.fs2_workspace_bytes(h, B, L, T, C.byref(p), C.byref(s)) == 0
                    assert p.value > 0 and s.value > 0, (name, B, L, T)
                    size[B, L, T] = (p.value, s.value)
        lib.fs2_destroy(h)
        for (B, L, T), (p, s) in size.items():
            assert p == size[B, L, Ts[0]][0], (name, B, L, T)  # persist: no T in it
            bigger = [(b2, L, T) for b2 in Bs if b2 > B] + [(B, l2, T) for l2 in Ls if l2 > L] + [(B, L, t2) for t2 in Ts if t2 > T]
            for k in bigger:
                assert size[k][0] >= p and size[k][1] >= s, (name, (B, L, T), k)


def test_recipe_with_five_priors_fits_the_abi(lib):
    # scripts/train.sh:27,49 of the reference: four variances, five priors
    names = ["pitch", "energy", "snr", "srmr"]
    priors = ["energy", "duration", "snr", "pitch", "srmr"]
    stats = {v: {"min": -3.0, "max": 3.0, "mean": 0.0, "std": 1.0} for v in names}
    stats.update({f"{p}_prior": {"min": -2.0, "max": 2.0, "mean": 0.0, "std": 1.0} for p in priors})
    cfg = Fs2Config(variances=names, variance_levels=["frame"] * 4, variance_transforms=["none"] * 4,
                    variance_nlayers=[5] * 4, variance_kernel_size=[3] * 4, priors=priors, stats=stats,
                    decoder_layers=6, decoder_kernel_sizes=[9] * 6, duration_nlayers=5,
                    encoder_depthwise_conv=False, decoder_depthwise_conv=False)
    st, h = _create(lib, cfg, _lib.FS2_BF16)
    assert st == 0, lib.fs2_last_error(h)
    lib.fs2_destroy(h)
    cfg.priors = [f"p{i}" for i in range(9)]
    with pytest.raises(ValueError, match="too many priors"):
        _lib.config_to_c(cfg, _lib.FS2_BF16)


def test_load_weight_checks_names_and_shapes(lib):
    cfg = preset("ref-default")
    st, h = _create(lib, cfg)
    assert st == 0
    sd = synth_state_dict(cfg, 0)

    def load(name, arr):
        a = np.ascontiguousarray(arr, np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        return lib.fs2_load_weight(h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim)

    # every tensor of the reference state_dict (reference key names) is accepted ...
    for name, shape in state_dict_spec(cfg).items():
        assert load(name, sd[name]) == 0, name
    # ... off-path / misspelled names and wrong shapes are refused
    assert load("fastdiff_linear.0.weight", np.zeros((256, 256))) == 4
    assert load("encoder.layers.0.conv1.weight", np.zeros((1024, 256, 5))) == 4  # dense key on a depth-wise config
    assert load("linear.weight", np.zeros((80, 255))) == 4
    assert b"shape mismatch" in lib.fs2_last_error(h)
    # decode before encode is a state error, not a crash
    out = _lib.Fs2OutputsC()
    assert lib.fs2_decode(h, C.byref(out), None) == 5
    lib.fs2_destroy(h)


def test_product_path_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from lightningfastspeech2_amd.model import FastSpeech2
    cfg = preset("ref-default")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FastSpeech2(cfg, synth_state_dict(cfg, 0))


def test_product_package_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lightningfastspeech2_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dp, f)).read()
                assert "oracle_cpu" not in text and "import oracle" not in text and "from oracle" not in text, f


def test_split_k_choice_is_a_pure_shape_function(lib):
    """fs2_op_gemm_splitk_choice runs on the host: the shapes the training step meets.  A long reduction over few row tiles
    splits (the encoder-side data-gradient convs), launches that already fill the chip or reduce over a short K do not."""
    BF16, F32 = 1, 0
    f = lib.fs2_op_gemm_splitk_choice
    assert f(BF16, 8192, 256, 1024, 9, 256) == 4      # C2 encoder conv1 data gradient: 64 row tiles x 4 = one round of 256 CUs
    assert f(BF16, 2048, 1024, 4096, 9, 256) == 4     # C5, 8 utterances per GPU
    assert f(BF16, 49152, 256, 1024, 9, 1536) == 1    # decoder: 384 row tiles already
    assert f(BF16, 8192, 1024, 256, 1, 8192) == 1     # short reduction
    assert f(BF16, 8192, 128, 1024, 9, 256) == 1      # narrower than the slab kernel's column tile
    assert f(BF16, 8192, 256, 1024, 2, 256) == 1      # even tap count: not a slab-kernel conv
    for dt in (F32, BF16):
        for args in ((8192, 256, 1024, 9, 256), (2048, 1024, 4096, 9, 256), (300, 256, 2048, 1, 300)):
            k = f(dt, *args)
            assert k >= 1 and (args[2] // (64 if dt == BF16 else 32)) % k == 0


def test_knob_setter_rejects_undefined_values(lib):
    """fs2_op_set_gemm_variant takes closed ranges - a typo in FS2_GEMM_KNOBS is an error, not a silent default; the
    switches removed in r05 (measured-slower forms: 1211, 211, 1301 / 1302, 301, 311 and their "off" values) are undefined now, and
    so is 2 (the 128x256 DMA-ring GEMM, moved to tools/probes/gemm_forms)."""
    FS2_OK, FS2_ERR_ARG = 0, lib.fs2_op_set_gemm_variant(-1)
    assert FS2_ERR_ARG != FS2_OK
    for bad in (1300, 1301, 1302, 1319, 1322, 1399, 1403, 1205, 1210, 1211, 1299, 1102, 1002, 910, 802, 702, 502, 310, 311, 300, 301, 210, 211, 222, 203, 250, 251, 252, 253, 8, 2, 100000):
        assert lib.fs2_op_set_gemm_variant(bad) == FS2_ERR_ARG, bad
    # the defaults (each is a defined value) leave the process as it was
    for ok in (0, 202, 201, 221, 230, 231, 500, 701, 801, 909, 904, 1001, 1100, 1203, 1321, 1340, 1341, 1401, 1501):
        assert lib.fs2_op_set_gemm_variant(ok) == FS2_OK, ok


def test_vocoder_knob_setters_reject_undefined_values(lib):
    """fs2_op_set_vocoder_fused_resblock takes the values the engine gives a meaning to (0, 1, 2, 4, 7, 9, 50..100),
    fs2_op_set_vocoder_lds_limit 0..150 KiB; anything else is FS2_ERR_ARG and leaves the knob as it was (read back through the
    host-side picker, which reads the calling thread's knobs)."""
    FS2_OK, FS2_ERR_ARG = _lib.FS2_OK, _lib.FS2_ERR_ARG
    d = (C.c_int32 * 3)(1, 3, 5)
    form = lambda: lib.fs2_op_vocoder_resblock_form(_lib.FS2_BF16, 64, 3, d, 3)
    tile = lambda: lib.fs2_op_vocoder_conv_tile(_lib.FS2_BF16, 256, 256, 11, 5, 0, 0, None)
    try:
        assert lib.fs2_op_set_vocoder_fused_resblock(4) == FS2_OK and form() == 808
        for bad in (-1, -50, 3, 5, 6, 8, 10, 25, 49, 101, 150, 1000, 2 ** 31 - 1, -2 ** 31):
            assert lib.fs2_op_set_vocoder_fused_resblock(bad) == FS2_ERR_ARG, bad
            assert form() == 808, bad
        for ok in (0, 1, 2, 4, 7, 9, 50, 60, 85, 100):
            assert lib.fs2_op_set_vocoder_fused_resblock(ok) == FS2_OK, ok
        assert lib.fs2_op_set_vocoder_lds_limit(150) == FS2_OK and tile() == 14
        for bad in (-1, -150, 151, 152, 1024, 2 ** 31 - 1, -2 ** 31):
            assert lib.fs2_op_set_vocoder_lds_limit(bad) == FS2_ERR_ARG, bad
            assert tile() == 14, bad
        for ok in (0, 1, 12, 76, 110, 149, 150):
            assert lib.fs2_op_set_vocoder_lds_limit(ok) == FS2_OK, ok
    finally:
        assert lib.fs2_op_set_vocoder_fused_resblock(1) == FS2_OK and lib.fs2_op_set_vocoder_lds_limit(0) == FS2_OK
    assert form() == 408 and tile() == 8


def test_library_has_no_mutable_tuning_globals():
    """SURVEY 8b "no global state (one handle per device)" / VERDICT r04 item 6: the A/B switches live in a per-engine / per-thread
    `fs2::Tuning`, not in process-wide `int g_*` variables every engine and pipeline thread reads unsynchronised.  By `nm`: no
    defined data symbol named fs2::g_* except the read-only device zero page."""
    import subprocess
    from lightningfastspeech2_amd import _lib
    out = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    bad = []
    for line in out.splitlines():
        parts = line.split(None, 2)
        if len(parts) == 3 and parts[1] in "bBdD" and "fs2::g_" in parts[2] and "(" not in parts[2] and "g_zero_page" not in parts[2]:
            bad.append(parts[2])
    assert not bad, bad


# ---- the pointer converter: a tensor or a stream goes into a call as it is ----------------------------------------------------
def test_converter_sits_on_every_plain_pointer_parameter_and_on_no_other(lib):
    """By the header's own text: a parameter that is a single-star pointer to a scalar, to void or to an opaque handle carries
    _lib.DevPtr; values, `const char*` names, struct pointers and `**` out-handles keep the type the parser gave them."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    parsed = _lib.parse_header(_lib.HEADER_PATH)
    n = 0
    for m in re.finditer(r"\b(fs2_[a-z0-9_]+)\s*\(([^()]*)\)", text):
        name, params = m.groups()
        for i, prm in enumerate([] if params.strip() == "void" else params.split(",")):
            base, stars = re.fullmatch(r"\s*(\w+)\s*(\**)\s*\w*\s*", re.sub(r"\bconst\b", " ", prm)).groups()
            plain = stars == "*" and base not in parsed.structs and not (base == "char" and "const" in prm)
            got = getattr(lib, name).argtypes[i]
            assert (got is _lib.DevPtr) == plain and (plain or got.__name__ == parsed.functions[name][1][i].__name__), (name, i, prm)
            n += plain
    assert n >= 500  # the operator entry points alone take several hundred tensors


def _identity():
    """memcpy(dst, src, 0) returns dst: a host function that hands a pointer argument back, typed with the converter"""
    f = C.CDLL(None).memcpy
    f.restype, f.argtypes = C.c_void_p, [_lib.DevPtr, _lib.DevPtr, C.c_size_t]
    src = C.c_int(0)
    return lambda x: f(x, C.byref(src), 0)


def test_converter_passes_each_kind_of_argument_as_a_64_bit_pointer():
    ident = _identity()
    high = 0x7F12_3456_789A  # above 4 GiB: a converter that hands ctypes a bare int would pass a C int
    word, arr = C.c_int(5), (C.c_int32 * 4)()

    class Stream:
        cuda_stream = high + 16

    class Tensor:
        def data_ptr(self):
            return high + 32

    assert ident(None) is None
    assert ident(C.c_void_p(high)) == high and ident(high) == high
    assert ident(C.byref(word)) == C.addressof(word) and ident(C.pointer(word)) == C.addressof(word)
    assert ident(arr) == C.addressof(arr)
    assert ident(Stream()) == high + 16 and ident(Tensor()) == high + 32
    a = np.zeros(3, np.float32)
    assert ident(a.ctypes.data_as(C.c_void_p)) == a.ctypes.data
    with pytest.raises(C.ArgumentError):
        ident(1.5)  # what c_void_p refuses stays refused


def test_host_conversion_takes_tensors_directly(lib):
    """One real call through 64-bit heap pointers (fs2_host_f32_to_f16 is host code): tensors passed as they are, the same call
    through explicit pointers, and the storage rule in torch give the same bits; so does a temporary passed inline."""
    import torch
    import _f16
    x = _f16.edge_values()
    n = x.numel()
    direct, explicit, inline = (torch.full((n,), 0x5A5A, dtype=torch.int16) for _ in range(3))
    assert lib.fs2_host_f32_to_f16(x, direct, n) == 0
    src, dst = x.data_ptr(), explicit.data_ptr()
    assert lib.fs2_host_f32_to_f16(C.c_void_p(src), C.c_void_p(dst), n) == 0
    assert lib.fs2_host_f32_to_f16(x.clone(), inline, n) == 0  # the temporary lives until the call returns
    want = _f16.f16_bits(x)
    assert torch.equal(direct, want) and torch.equal(explicit, want) and torch.equal(inline, want)


def test_check_names_the_handle_kind(lib):
    """_lib.check formats every handle's failure alike; last_error picks the entry point that holds the handle's message."""
    with pytest.raises(RuntimeError, match=r"^fs2 set_debug failed \(1\): ") as e:
        _lib.check(1, None, "set_debug")
    assert str(e.value) == f"fs2 set_debug failed (1): {lib.fs2_status_string(1).decode()}"
    with pytest.raises(AttributeError):
        _lib.check(1, C.c_void_p(1), "x", last_error="fs2_no_such_last_error")
    _lib.check(0, C.c_void_p(1), "x", last_error="fs2_no_such_last_error")  # FS2_OK: nothing is looked up
