"""ctypes binding of include/tssplat_amd.h (libtssplat_amd.so), read from the header itself.

The library is the product; this file is plumbing.  There is deliberately no
Python/CPU fallback: if the shared library cannot be loaded, importing the
operator surface raises.

Nothing of the header is restated here.  :func:`read_header` reads the structs, the constants and the declarations of
include/tssplat_amd.h at import -- the header as it is written and no more general C; what it does not understand is an
``ImportError``, never a guess -- and the Structure classes, ``SIGNATURES`` and the ``TSAMD_*`` names below come from that reading.
A new entry point is declared in the header and defined in csrc/; there is no Python table to extend.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import re

from . import _build

_lib = None


class TsamdError(RuntimeError):
    """A C-ABI call failed (the reference surfaces native failures as RuntimeError too,
    /root/reference/tssplat_ext/tet_spheres/cudaUtils.h:10-44)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"tssplat_amd error {code}: {message}")
        self.code = code


# ---- the reader ----
Header = collections.namedtuple("Header", "structs opaque constants functions")
Header.__doc__ = """What include/tssplat_amd.h declares: ``structs`` name -> Structure class, ``opaque`` the names of the handle types,
``constants`` name -> int (enum members and integer #defines), ``functions`` name -> (restype, [(parameter, ctype), ...])."""

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16,
            "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_CPLUSPLUS = re.compile(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b", re.S | re.M)     # extern "C" { and its }
_DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*(\w+)[ \t]*(.*?)[ \t]*$", re.M)
_DEFINE = re.compile(r"(TSAMD_\w+)\s+(-?(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0))")
_MEMBER = re.compile(r"\s*(TSAMD_\w+)\s*=\s*(-?[0-9]+)\s*")
_ITEM = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s+(\w+)"                           # 1, 2: an opaque type
                   r"|typedef\s+(struct|enum)\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)"       # 3-6: a struct or the enum
                   r"|([^;(){}]+)\(([^;(){}]*)\))\s*;")                               # 7, 8: a function
_TYPE = re.compile(r"(const\s+)?(\w+)\b\s*(.+)", re.S)
_NAME = re.compile(r"((?:\s*\*)*)\s*(\w+)\s*")
_END = re.compile(r"\s*\Z")


def _flat(text: str) -> str:
    return " ".join(text.split())[:200]


def _declare(text: str, where: str) -> list:
    """``const int32_t *a, *b`` -> [(True, "int32_t", 1, "a"), (True, "int32_t", 1, "b")]: const, base type, pointer depth, name."""
    m = _TYPE.fullmatch(text.strip())
    names = [_NAME.fullmatch(part) for part in m[3].split(",")] if m else [None]
    if not all(names):
        raise ImportError(f"{where}: cannot read '{_flat(text)}'")
    return [(bool(m[1]), m[2], n[1].count("*"), n[2]) for n in names]


def _ctype(decl: tuple, where: str, header: Header, parameter: bool):
    """The ctypes type of one declarator.  A pointer to a parsed struct is POINTER(its class); ``const char *`` is c_char_p; a
    pointer is c_void_p when it is ``void *``, points to an opaque struct, is named ``*_dev`` or -- for a parameter -- points to
    a const scalar (input arrays: callers pass addresses); ``opaque **`` is POINTER(c_void_p); any other ``T *`` / ``T **`` is typed."""
    const, base, depth, name = decl
    if depth == 0 and base in _SCALARS:
        return _SCALARS[base]
    if depth == 1 and base in header.structs:
        return C.POINTER(header.structs[base])
    if depth == 1 and base == "char" and const:
        return C.c_char_p
    if depth == 1 and (base == "void" or base in header.opaque):
        return C.c_void_p
    if depth == 2 and base in header.opaque:
        return C.POINTER(C.c_void_p)
    if base not in _SCALARS or not 1 <= depth <= 2:
        raise ImportError(f"{where}: no ctypes type for '{'const ' if const else ''}{base} {'*' * depth}{name}'")
    if depth == 1 and (name.endswith("_dev") or (parameter and const)):
        return C.c_void_p
    return C.POINTER(_SCALARS[base]) if depth == 1 else C.POINTER(C.POINTER(_SCALARS[base]))


def read_header(text: str, classes: dict | None = None, path: str = "header") -> Header:
    """Read the text of include/tssplat_amd.h.  ``classes``: C struct name -> a ``ctypes.Structure`` subclass without ``_fields_``
    that is to receive them (a struct without one gets a class of its own name)."""
    header = Header({}, set(), {}, {})
    guard = []

    def directive(m):
        word, rest = m[1], m[2]
        value = _DEFINE.fullmatch(rest) if word == "define" else None
        if value:
            header.constants[value[1]] = int(value[2], 0)
        elif word == "ifndef":
            guard.append(rest)
        elif not (word in ("endif", "include") or (word == "define" and rest in guard)):     # (#define GUARD: the include guard)
            raise ImportError(f"{path}: cannot read '#{word} {_flat(rest)}'")
        return ""

    text = _DIRECTIVE.sub(directive, _CPLUSPLUS.sub("", _COMMENT.sub(" ", text)))
    pos = 0
    while not _END.match(text, pos):
        m = _ITEM.match(text, pos)
        if not m or m[1] != m[2] or m[4] != m[6]:
            raise ImportError(f"{path}: cannot read the declaration '{_flat(text[pos:].split(';')[0])}'")
        pos = m.end()
        if m[1]:
            header.opaque.add(m[1])
        elif m[3] == "enum":
            for part in m[5].split(","):
                member = _MEMBER.fullmatch(part)
                if not member:
                    raise ImportError(f"{path}: {m[4]}: cannot read the member '{_flat(part)}'")
                header.constants[member[1]] = int(member[2])
        elif m[3] == "struct":
            where = f"{path}: {m[4]}"
            fields = [(d[3], _ctype(d, where, header, False)) for line in m[5].split(";") if line.strip() for d in _declare(line, where)]
            cls = (classes or {}).get(m[4]) or type(m[4], (C.Structure,), {})
            cls._fields_ = fields                         # in the header's order
            header.structs[m[4]] = cls
        else:
            head = _declare(m[7], path)
            if len(head) != 1:
                raise ImportError(f"{path}: cannot read the declaration '{_flat(m[0])}'")
            *result, name = head[0]
            where = f"{path}: {name}"
            params = [] if m[8].strip() == "void" else [d for part in m[8].split(",") for d in _declare(part, where)]
            restype = None if tuple(result) == (False, "void", 0) else _ctype((*result, name), where, header, False)
            header.functions[name] = (restype, [(d[3], _ctype(d, where, header, True)) for d in params])
    missing = sorted(set(classes or {}) - set(header.structs))
    if missing:
        raise ImportError(f"{path}: does not declare the structs {missing}")
    return header


# ---- the header's structs as classes: the fields are the header's, in its order ----
class Options(C.Structure):
    """``tsamd_options``"""


class PlanInfo(C.Structure):
    """``tsamd_plan_info``"""

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PartitionInfo(C.Structure):
    """``tsamd_partition_info``"""


class TileView(C.Structure):
    """``tsamd_tile_view``: host pointers, typed -- tests/tile_emulator.py indexes them."""


class BlendPlanStruct(C.Structure):
    """``tsamd_blend_plan``: device pointers and sizes of a blend plan (tssplat_amd/dr.py: BlendPlan)."""


class SmoothMeshStruct(C.Structure):
    """``tsamd_smooth_mesh``: sizes and device pointers of a vertex adjacency (tssplat_amd/smooth.py: VertexAdjacency)."""


with open(_build.HEADER) as _fh:
    HEADER = read_header(_fh.read(), {"tsamd_options": Options, "tsamd_plan_info": PlanInfo, "tsamd_partition_info": PartitionInfo,
                                      "tsamd_tile_view": TileView, "tsamd_blend_plan": BlendPlanStruct,
                                      "tsamd_smooth_mesh": SmoothMeshStruct}, "include/tssplat_amd.h")

# Parameters whose type is NOT what _ctype's rule gives, keyed (function, parameter); tests/test_capi_bindings.py fails an entry
# that names nothing in the header or that the rule has caught up with.
_FLOATS, _INTS = C.POINTER(C.c_float), C.POINTER(C.c_int32)
EXCEPTIONS = {
    # the schedule of a launch: host arrays that callers pass as ctypes arrays, so the element type is checked
    ("tsamd_train_loop_launch", "c1"): _FLOATS, ("tsamd_train_loop_launch", "c2"): _FLOATS,
    ("tsamd_train_loop_launch", "order"): _INTS, ("tsamd_train_loop_launch", "grad_limit"): _FLOATS,
    # host output arrays that callers pass as ndarray.ctypes.data, a plain address
    ("tsamd_extract_surface", "surface_vid"): C.c_void_p, ("tsamd_extract_surface", "faces"): C.c_void_p,
    # the same: four numpy arrays by address
    ("tsamd_grid_layout", "offsets_out"): C.c_void_p, ("tsamd_grid_layout", "resolution_out"): C.c_void_p,
    ("tsamd_grid_layout", "hashed_out"): C.c_void_p, ("tsamd_grid_layout", "scale_out"): C.c_void_p,
}

# every symbol include/tssplat_amd.h declares: name -> (restype, argtypes)
SIGNATURES = {name: (restype, [EXCEPTIONS.get((name, p), t) for p, t in params]) for name, (restype, params) in HEADER.functions.items()}
globals().update(HEADER.constants)          # every TSAMD_* enum member and integer #define by name: _capi.TSAMD_SMOOTH_TAUBIN
ABI_VERSION = HEADER.constants["TSAMD_ABI_VERSION"]


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True):
    """Load libtssplat_amd.so (building it in-tree first if hipcc is around and it is stale/missing)."""
    global _lib
    if _lib is not None:
        return _lib
    # The host framework's HIP runtime must be in the process first: torch bundles its own
    # libamdhip64.so.7, and a second copy (from /opt/rocm) loaded ahead of it leaves one of the
    # two runtimes without devices ("no HIP device is visible").
    import torch  # noqa: F401
    path = _build.LIB
    override = os.environ.get("TSSPLAT_AMD_LIB")       # experiment builds (tssplat_amd._build.build_variant)
    if override:
        path, build_if_missing = override, False
    if build_if_missing:
        try:
            path = _build.build()
        except Exception:
            if not os.path.exists(path):
                raise
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m tssplat_amd._build` (needs hipcc, --offload-arch=gfx950). "
            "tssplat_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.tsamd_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.tsamd_abi_version()}, these bindings are written for {ABI_VERSION} "
                          "(include/tssplat_amd.h: TSAMD_ABI_VERSION) -- rebuild the library")
    _lib = lib
    return lib


_ext_module = None


def autograd_ext(build_if_missing: bool = True):
    """The C++ torch extension (csrc/torch_autograd.cpp + csrc/torch_exchange.cpp, tssplat_amd/_tsamd_autograd.so): the autograd
    nodes of the energy and the energy exchange's helper thread, wired to the entry points of the library loaded above.  Like
    :func:`load` there is no fallback: if the extension cannot be built or imported, this raises."""
    global _ext_module
    if _ext_module is not None:
        return _ext_module
    lib = load()
    if build_if_missing:
        try:
            _build.build_torch_ext()
        except Exception:
            if not os.path.exists(_build.TORCH_EXT):
                raise
    if not os.path.exists(_build.TORCH_EXT):
        raise ImportError(
            f"{_build.TORCH_EXT} is missing: build it with `python -m tssplat_amd._build` (needs g++ and the torch headers). "
            "tssplat_amd has no Python fallback for it.")
    import importlib
    ext = importlib.import_module("tssplat_amd._tsamd_autograd")
    addr = lambda fn: C.cast(fn, C.c_void_p).value
    ext.set_entry_points(addr(lib.tsamd_graph_launch), addr(lib.tsamd_forward_backward), addr(lib.tsamd_last_error))
    _ext_module = ext
    return ext


def check(rc: int) -> None:
    if rc != 0:
        raise TsamdError(rc, load().tsamd_last_error().decode("utf-8", "replace"))


def make_options(**kw) -> Options:
    o = Options()
    o.struct_size = C.sizeof(Options)
    o.abi_version = ABI_VERSION
    o.device = -1
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown tsamd option {k!r}")
        setattr(o, k, int(v))
    return o
