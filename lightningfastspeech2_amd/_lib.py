"""ctypes binding of libfs2_hip.so (C ABI declared in include/fs2.h).

The product path has no CPU fallback: if the HIP library is missing or does not export the full
ABI, importing the engine raises.  ``torch`` is imported first on purpose — it loads the ROCm
runtime (libamdhip64.so.7) this library then shares, so torch device pointers and streams are
valid in our launches.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import torch  # (must precede the dlopen below)

_HERE = os.path.dirname(os.path.abspath(__file__))
# FS2_LIB: alternative build of the same ABI (kernel A/B experiments); default = the in-tree library
LIB_PATH = os.environ.get("FS2_LIB") or os.path.join(_HERE, "libfs2_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fs2.h")


class Fs2LibraryError(RuntimeError):
    pass


# The closed type table: scalars passed or stored by value, and what a pointer may point to besides a type the header declares.
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "int8_t", "int16_t", "uint16_t"}


def parse_header(src: str = HEADER_PATH):
    """include/fs2.h (a path, or header text: anything with a newline in it) -> its constants {name: int}, structs {C name:
    ctypes.Structure} and functions {name: (restype, argtypes)}.  The header is the single source of the binding, so whatever
    this grammar cannot type is an Fs2LibraryError naming the declaration, never a default."""
    if "\n" not in src:
        with open(src) as f:
            src = f.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    loose = set(re.findall(r"\b(fs2_[a-z0-9_]+)\s*\(", text))  # every name that looks declared: none may end up unbound
    consts = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(FS2_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M)}

    def const(word, where):
        if word not in consts and not re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", word):
            raise Fs2LibraryError(f"include/fs2.h: {where}: {word!r} is neither an integer nor a constant declared above it")
        return consts[word] if word in consts else int(word, 0)

    def enum(m):
        nxt = 0
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, _, val = (s.strip() for s in item.partition("="))
            consts[name] = nxt = const(val, name) if val else nxt
            nxt += 1
        return " "

    def struct(m):
        name, fields = m.group(1), []
        for stmt in filter(None, (s.strip() for s in m.group(2).split(";"))):
            head = re.fullmatch(r"(?:const\s+)?(\w+)\b(.*)", stmt, re.S)
            base, rest = head.groups() if head else (None, "")
            for decl in rest.split(","):
                d = re.fullmatch(r"\s*(\**)\s*(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)", decl)
                t = d and (C.c_void_p if d.group(1) else C.c_char if base == "char" else _SCALARS.get(base))
                if not t:
                    raise Fs2LibraryError(f"include/fs2.h: struct {name}: field {stmt!r} is outside the binding's type table")
                for dim in reversed(re.findall(r"\w+", d.group(3))):
                    t = t * const(dim, f"struct {name}.{d.group(2)}")
                fields.append((d.group(2), t))
        structs[name] = type(name, (C.Structure,), {"_fields_": fields})
        return " "

    def ctype(decl, fn, ret=False):
        m = re.fullmatch(r"\s*(\w+)\s*((?:\*\s*)*)(\w+)?\s*", re.sub(r"\bconst\b", " ", decl))
        base, stars = (m.group(1), m.group(2).count("*")) if m and not (ret and m.group(3)) else (None, 0)
        if not stars:
            t = _SCALARS.get(base)
        elif base == "char" and stars == 1 and re.search(r"\bconst\b", decl):
            t = C.c_char_p
        elif base in structs and stars == 1:
            t = C.POINTER(structs[base])
        elif base in opaque and stars == 2:
            t = C.POINTER(C.c_void_p)
        else:
            t = C.c_void_p if base in _POINTEES or base in opaque or base in structs else None
        if t is None and not (ret and base == "void" and not stars):
            raise Fs2LibraryError(f"include/fs2.h: {fn}: {' '.join(decl.split())!r} is outside the binding's type table")
        return t

    text = re.sub(r"#[ \t]*ifdef[ \t]+__cplusplus.*?#[ \t]*endif", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r"\benum\s+\w*\s*\{(.*?)\}\s*;", enum, text, flags=re.S)
    structs, funcs = {}, {}
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    opaque = set(re.findall(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", text))
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", " ", text)
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(fs2_[a-z0-9_]+)\s*\(([^()]*)\)", stmt, re.S)
        if not m:
            raise Fs2LibraryError(f"include/fs2.h: not a prototype the binding can parse: {' '.join(stmt.split())!r}")
        ret, name, params = m.groups()
        funcs[name] = (ctype(ret, name, ret=True), [] if params.strip() == "void" else [ctype(p, name) for p in params.split(",")])
    if set(funcs) != loose:
        raise Fs2LibraryError(f"include/fs2.h: declared in a form the binding does not parse: {sorted(loose - set(funcs))}")
    return SimpleNamespace(constants=consts, structs=structs, functions=funcs)


# The binding is generated: every constant of the header under its own name (FS2_K_<X> also as K_<X>), every struct as
# <CamelCase of its C name>C, every function typed in load().  A new entry point needs nothing here.
_HEADER = parse_header()
globals().update(_HEADER.constants)
globals().update({n[4:]: v for n, v in _HEADER.constants.items() if n.startswith("FS2_K_")})
globals().update({n.title().replace("_", "") + "C": t for n, t in _HEADER.structs.items()})
BGemmDescC = _HEADER.structs["fs2_bgemm_desc"]  # the name this struct had before the binding was generated


def declared_symbols(header_path: str = HEADER_PATH):
    """Every function include/fs2.h declares (used to verify the library exports the full ABI)."""
    return sorted((_HEADER if header_path == HEADER_PATH else parse_header(header_path)).functions)


class DevPtr:
    """The argtype load() gives every parameter the header types as a plain `void*`: a tensor (anything with data_ptr()), a
    torch.cuda.Stream (anything with .cuda_stream), None, or whatever c_void_p takes (opaque handles, byref, ctypes arrays and
    pointers, ints) goes into the call as a 64-bit pointer.  It converts and does not validate: strided views and host pointers
    are legitimate arguments.  The argument stays referenced by the caller's frame for the call, so a temporary is safe here."""

    @classmethod
    def from_param(cls, obj):
        try:
            return _VOIDP(obj.data_ptr())  # a c_void_p, never the bare int: ctypes would pass that as a C int
        except AttributeError:
            return _VOIDP.from_param(getattr(obj, "cuda_stream", obj))


_VOIDP = C.c_void_p
_lib = None


def load():
    """dlopen libfs2_hip.so and type its entry points (plain void* parameters as DevPtr).  Raises Fs2LibraryError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Fs2LibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in _HEADER.functions if not hasattr(lib, s)]
    if missing:
        raise Fs2LibraryError(f"{LIB_PATH} does not export: {missing}")
    for name, (restype, argtypes) in _HEADER.functions.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, [DevPtr if t is C.c_void_p else t for t in argtypes]
    if lib.fs2_abi_version() != FS2_ABI_VERSION:
        raise Fs2LibraryError("libfs2_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(status: int, engine=None, what: str = "", last_error=None, lib=None):
    """Raise on a status other than FS2_OK.  engine = the handle whose message to append; last_error = the name of the
    entry point that returns it, for handles other than the engine's ("fs2_voc_last_error", "fs2_mel_last_error")."""
    if status == FS2_OK:
        return
    lib = lib or load()
    msg = lib.fs2_status_string(status).decode()
    if engine:
        detail = getattr(lib, last_error or "fs2_last_error")(engine).decode()
        if detail:
            msg = f"{msg}: {detail}"
    raise RuntimeError(f"fs2 {what} failed ({status}): {msg}")


class Handle:
    """Base of the five wrappers that own an opaque handle of include/fs2.h.  A subclass names its family (``_prefix``: "fs2",
    "fs2_voc", "fs2_sdp", "fs2_mel", "fs2_fd" - the base finds ``<prefix>_last_error`` / ``_load_weight`` / ``_finalize`` /
    ``_destroy`` from it), makes its own ``<prefix>_create`` call into ``self.handle`` and, when anything after that call fails,
    calls ``close()`` before it re-raises.  ``_label`` and ``_load_what`` only word the RuntimeError of ``_check``."""
    _prefix = "fs2"
    _label = ""
    _load_what = "load_weight({})"

    def __init__(self, lib=None):
        self.lib = lib or load()
        self.handle = C.c_void_p()
        self._ws = None

    def _fn(self, what):
        return getattr(self.lib, f"{self._prefix}_{what}")

    def _check(self, status, what):
        check(status, self.handle, self._label + what, f"{self._prefix}_last_error", self.lib)

    def close(self):
        """Destroy the handle; harmless when called again (or on an object whose constructor never got that far)."""
        if getattr(self, "handle", None):
            handle, self.handle = self.handle, C.c_void_p()
            self._fn("destroy")(handle)  # (fs2_voc_destroy returns void: no result is looked at for any family)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, names, state_dict):
        """``<prefix>_load_weight`` for every name (tensors and arrays alike go in as contiguous float32), then
        ``<prefix>_finalize``."""
        load_weight = self._fn("load_weight")
        for name in names:
            v = state_dict[name]
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().float().numpy()
            a = np.ascontiguousarray(v, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(load_weight(self.handle, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim), self._load_what.format(name))
        self._check(self._fn("finalize")(self.handle), "finalize")

    def _workspace(self, nbytes: int):
        """The handle's grow-only device workspace (uint8 on ``self.device``), at least ``nbytes`` long."""
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None  # (released before the larger one is asked for)
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws


def config_to_c(cfg, dtype: int) -> Fs2ConfigC:
    """lightningfastspeech2_amd.config.Fs2Config -> fs2_config."""
    from .config import DVECTOR_DIM, PE_MAX_LEN
    c = Fs2ConfigC()
    c.abi_version = FS2_ABI_VERSION
    c.dtype = dtype
    c.n_phones = cfg.n_phones
    c.hidden = cfg.hidden
    c.n_mels = cfg.n_mels
    c.dvec_dim = DVECTOR_DIM
    c.max_frames = cfg.max_frames
    c.pe_len = PE_MAX_LEN
    if cfg.encoder_layers > FS2_MAX_LAYERS or cfg.decoder_layers > FS2_MAX_LAYERS:
        raise ValueError("too many layers for the C ABI")
    if len(cfg.variances) > FS2_MAX_VARIANCES:
        raise ValueError("too many variances for the C ABI")
    c.enc_layers, c.enc_heads = cfg.encoder_layers, cfg.encoder_head
    c.enc_filter, c.enc_depthwise = cfg.encoder_conv_filter_size, int(cfg.encoder_depthwise_conv)
    for i in range(cfg.encoder_layers):
        c.enc_kernels[i] = cfg.encoder_kernel_sizes[i]
    c.dec_layers, c.dec_heads = cfg.decoder_layers, cfg.decoder_head
    c.dec_filter, c.dec_depthwise = cfg.decoder_conv_filter_size, int(cfg.decoder_depthwise_conv)
    for i in range(cfg.decoder_layers):
        c.dec_kernels[i] = cfg.decoder_kernel_sizes[i]
    c.n_variances = len(cfg.variances)
    for i, v in enumerate(cfg.variances):
        name = v.encode()
        if len(name) >= FS2_NAME_LEN:
            raise ValueError("variance name too long")
        c.var_names[i].value = name
        c.var_nlayers[i] = cfg.variance_nlayers[i]
        c.var_kernel[i] = cfg.variance_kernel_size[i]
        cwt = cfg.is_cwt(i)  # the CWT head bucketises its recomposed log-domain signal directly (model.py:427-428)
        c.var_cwt[i] = int(cwt)
        c.var_level[i] = int(cfg.is_phone_level(i))
        c.var_mean[i] = 0.0 if cwt else cfg.stats[v]["mean"]
        c.var_std[i] = 1.0 if cwt else cfg.stats[v]["std"]
    c.var_filter, c.var_nbins = cfg.variance_filter_size, cfg.variance_nbins
    c.var_depthwise = int(cfg.variance_depthwise_conv)
    if len(cfg.priors) > FS2_MAX_PRIORS:
        raise ValueError("too many priors for the C ABI")
    c.n_priors = len(cfg.priors)
    for i, pr in enumerate(cfg.priors):
        c.prior_names[i].value = pr.encode()
    c.dur_nlayers, c.dur_kernel = cfg.duration_nlayers, cfg.duration_kernel_size
    c.dur_filter, c.dur_depthwise = cfg.duration_filter_size, int(cfg.duration_depthwise_conv)
    return c
