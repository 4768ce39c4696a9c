"""tssplat_amd/_capi.py reads its ctypes bindings from include/tssplat_amd.h.  CPU tier, no library load: the reader on small header
texts (every construct the header uses, each on its own, and every construct it must refuse), the pointer rule with its table of
exceptions, and the C compiler's own reading of the header -- sizes, offsets and constants -- against the classes and names here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tssplat_amd import _build, _capi

read = _capi.read_header
P = C.POINTER
STRUCTS = {"tsamd_options": _capi.Options, "tsamd_plan_info": _capi.PlanInfo, "tsamd_partition_info": _capi.PartitionInfo,
           "tsamd_tile_view": _capi.TileView, "tsamd_blend_plan": _capi.BlendPlanStruct, "tsamd_smooth_mesh": _capi.SmoothMeshStruct}


def refused(text: str, *names: str):
    """The reader refuses ``text`` with an ImportError that names the declaration."""
    with pytest.raises(ImportError) as err:
        read(text)
    for name in names:
        assert name in str(err.value), str(err.value)


# ---- the reader, construct by construct ----
def test_comma_declarators_scalars_and_pointers():
    h = read("typedef struct tsamd_a {\n    int32_t struct_size;\n    int64_t n_vertices, n_tets;\n    const int32_t *x_dev, *y;\n"
             "    double lo, hi;\n} tsamd_a;")
    assert h.structs["tsamd_a"]._fields_ == [("struct_size", C.c_int32), ("n_vertices", C.c_int64), ("n_tets", C.c_int64), ("x_dev", C.c_void_p),
                                             ("y", P(C.c_int32)), ("lo", C.c_double), ("hi", C.c_double)]
    assert issubclass(h.structs["tsamd_a"], C.Structure) and C.sizeof(h.structs["tsamd_a"]) == 8 + 2 * 8 + 2 * 8 + 2 * 8
    assert not h.functions and not h.constants and not h.opaque


def test_every_scalar_by_name():
    names = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32,
             "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    h = read("".join(f"{t} tsamd_f{i}({t} a, {t} *b);\n" for i, t in enumerate(names)))
    assert [h.functions[f"tsamd_f{i}"] for i in range(len(names))] == [(t, [("a", t), ("b", P(t))]) for t in names.values()]


def test_declaration_over_three_lines():
    h = read("int tsamd_f(const float *x_dev, int64_t n,\n            float c1,   double\n  c2,\n            void *stream);\n")
    assert h.functions == {"tsamd_f": (C.c_int, [("x_dev", C.c_void_p), ("n", C.c_int64), ("c1", C.c_float), ("c2", C.c_double), ("stream", C.c_void_p)])}


def test_void_parameter_list_and_return_types():
    h = read("const char *tsamd_text(void);\nint32_t tsamd_number( void );\nvoid tsamd_nothing(void);\nint64_t tsamd_bytes(int32_t n);")
    assert h.functions == {"tsamd_text": (C.c_char_p, []), "tsamd_number": (C.c_int32, []), "tsamd_nothing": (None, []),
                           "tsamd_bytes": (C.c_int64, [("n", C.c_int32)])}


def test_pointer_to_pointer_and_opaque_types():
    h = read("typedef struct tsamd_h tsamd_h;\nint tsamd_f(const tsamd_h *h, tsamd_h *g, tsamd_h **out, const int32_t **vid, int64_t *n, int32_t ** rows);")
    assert h.opaque == {"tsamd_h"}
    assert h.functions["tsamd_f"][1] == [("h", C.c_void_p), ("g", C.c_void_p), ("out", P(C.c_void_p)), ("vid", P(P(C.c_int32))), ("n", P(C.c_int64)),
                                         ("rows", P(P(C.c_int32)))]


def test_const_in_a_parameter_a_field_and_a_return_type():
    h = read("typedef struct tsamd_s { const uint16_t *rows; uint16_t *more; const float *w_dev; } tsamd_s;\n"
             "const char *tsamd_f(const float *x, float *y, const char *path, const void *masks_dev, const tsamd_s *s, float *out_dev);")
    s = h.structs["tsamd_s"]
    assert s._fields_ == [("rows", P(C.c_uint16)), ("more", P(C.c_uint16)), ("w_dev", C.c_void_p)]          # fields stay typed unless *_dev
    assert h.functions["tsamd_f"] == (C.c_char_p, [("x", C.c_void_p), ("y", P(C.c_float)), ("path", C.c_char_p), ("masks_dev", C.c_void_p),
                                                   ("s", P(s)), ("out_dev", C.c_void_p)])


def test_comments_of_both_styles_are_not_code():
    h = read("/* int tsamd_ghost(void); typedef struct x { int a[3]; } x;\n * closes with ); and opens struct x {\n */\n"
             "int tsamd_f(int32_t n /* not a parameter, ); */, float s); // struct x { ; int tsamd_other(void);\n"
             "#define TSAMD_N 4 /* not 5 */\n"
             "typedef struct tsamd_s {\n    int32_t a; /* struct x { */\n    // int32_t ghost;\n    int32_t b;\n} tsamd_s;\n")
    assert h.functions == {"tsamd_f": (C.c_int, [("n", C.c_int32), ("s", C.c_float)])} and h.constants == {"TSAMD_N": 4}
    assert [n for n, _ in h.structs["tsamd_s"]._fields_] == ["a", "b"]


def test_enum_members_and_integer_defines_are_constants():
    h = read("typedef enum tsamd_status {\n    TSAMD_OK = 0,\n    TSAMD_ERR_A = 1,  /* one */\n    TSAMD_ERR_B = 7\n} tsamd_status;\n"
             "#define TSAMD_ABI_VERSION 3\n#  define TSAMD_HEX 0x1F\n#define TSAMD_NEG -2\n#define TSAMD_ZERO 0\n")
    assert h.constants == {"TSAMD_OK": 0, "TSAMD_ERR_A": 1, "TSAMD_ERR_B": 7, "TSAMD_ABI_VERSION": 3, "TSAMD_HEX": 31, "TSAMD_NEG": -2, "TSAMD_ZERO": 0}


@pytest.mark.parametrize("line", ["#define TSAMD_PI 3.14", "#define TSAMD_NAME \"gfx950\"", "#define TSAMD_TWICE(x) 2", "#define TSAMD_SUM 1 + 2",
                                  "#define TSAMD_OCTAL 010", "#define TSAMD_ALIAS TSAMD_OTHER", "#define TSAMD_LONG 1L", "#define OTHER_PREFIX 1",
                                  "#define TSAMD_FLAG", "#if TSAMD_N > 2", "#pragma once", "#undef TSAMD_N"])
def test_a_define_that_is_no_integer_literal_is_refused(line):
    refused(f"int tsamd_f(void);\n{line}\n", line.split()[1] if len(line.split()) > 1 else line)


def test_include_guard_includes_and_the_cplusplus_blocks():
    h = read("#ifndef TSSPLAT_AMD_H\n#define TSSPLAT_AMD_H\n\n#include <stdint.h>\n\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
             "int tsamd_f(void);\n#ifdef __cplusplus\n}\n#endif\n#endif /* TSSPLAT_AMD_H */\n")
    assert h.functions == {"tsamd_f": (C.c_int, [])} and not h.constants and not h.structs
    refused("#ifndef A_H\n#define B_H\nint tsamd_f(void);\n#endif\n", "B_H")           # a bare #define that is not the guard's


@pytest.mark.parametrize("text, names", [
    ("typedef struct tsamd_s { int32_t n; float weights[4]; } tsamd_s;", ("tsamd_s", "weights")),                      # an array field
    ("int tsamd_visit(int64_t n, int (*callback)(int64_t), void *stream);", ("tsamd_visit",)),                         # a function pointer
    ("int tsamd_f(int64_t n, size_t bytes);", ("tsamd_f", "size_t")),                                                   # unknown type names
    ("int tsamd_f(unsigned int n);", ("tsamd_f", "unsigned")),
    ("typedef struct tsamd_s { long n; } tsamd_s;", ("tsamd_s", "long")),
    ("ssize_t tsamd_f(void);", ("tsamd_f", "ssize_t")),
    ("int tsamd_f(tsamd_undeclared *h);", ("tsamd_f", "tsamd_undeclared")),
    ("int tsamd_f(int32_t);", ("tsamd_f", "int32_t")),                                                                  # a parameter without a name
    ("int tsamd_f(void *stream, ...);", ("tsamd_f",)),
    ("int tsamd_f(float ***x);", ("tsamd_f", "x")),
    ("int tsamd_f(char *text);", ("tsamd_f", "text")),                                                                  # only const char * is a string
    ("typedef struct tsamd_a { int32_t n; } tsamd_a;\nint tsamd_f(tsamd_a by_value);", ("tsamd_f", "by_value")),
    ("typedef struct tsamd_a { int32_t n; } tsamd_a;\nint tsamd_f(tsamd_a **out);", ("tsamd_f", "out")),
    ("typedef struct tsamd_s { struct { int32_t a; } inner; } tsamd_s;", ("tsamd_s",)),
    ("typedef struct tsamd_s { int32_t a; } tsamd_t;", ("tsamd_s",)),
    ("typedef struct tsamd_s tsamd_t;", ("tsamd_s",)),
    ("typedef enum tsamd_e { TSAMD_A, TSAMD_B } tsamd_e;", ("tsamd_e", "TSAMD_A")),                                     # no implicit values
    ("typedef int32_t tsamd_index;", ("tsamd_index",)),
    ("struct tsamd_s { int32_t a; };", ("tsamd_s",)),
    ("extern int tsamd_counter;", ("tsamd_counter",)),
    ("static inline int tsamd_f(void) { return 0; }", ("tsamd_f",)),
    ("int tsamd_f(void)", ("tsamd_f",)),                                                                                # no semicolon
])
def test_what_the_reader_does_not_understand_is_an_import_error(text, names):
    refused("int tsamd_before(void);\n" + text + "\nint tsamd_after(void);\n", *names)


def test_structs_take_the_classes_they_are_given_and_the_headers_order():
    class Mesh(C.Structure):
        def total(self):
            return self.b + self.a

    text = "typedef struct tsamd_mesh { int64_t b; int32_t a; } tsamd_mesh;\ntypedef struct tsamd_other { float f; } tsamd_other;\nint tsamd_f(const tsamd_mesh *m, tsamd_other *o);"
    h = read(text, {"tsamd_mesh": Mesh})
    assert h.structs["tsamd_mesh"] is Mesh and Mesh._fields_ == [("b", C.c_int64), ("a", C.c_int32)] and Mesh(b=2, a=3).total() == 5
    other = h.structs["tsamd_other"]
    assert other.__name__ == "tsamd_other" and issubclass(other, C.Structure)
    assert h.functions["tsamd_f"][1] == [("m", P(Mesh)), ("o", P(other))]
    with pytest.raises(ImportError, match="tsamd_gone"):
        read(text, {"tsamd_gone": type("Gone", (C.Structure,), {})})


# ---- the bindings of the real header ----
def _header_text() -> str:
    with open(_build.HEADER) as fh:
        return fh.read()


def _without_comments(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_what_capi_offers():
    assert os.path.samefile(_build.HEADER, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tssplat_amd.h"))
    for name, cls in STRUCTS.items():
        assert issubclass(cls, C.Structure) and _capi.HEADER.structs[name] is cls
    assert {c.__name__ for c in STRUCTS.values()} == {"Options", "PlanInfo", "PartitionInfo", "TileView", "BlendPlanStruct", "SmoothMeshStruct"}
    assert set(_capi.HEADER.structs) == set(STRUCTS) and _capi.HEADER.opaque == {"tsamd_handle", "tsamd_graph", "tsamd_train_loop", "tsamd_surface"}
    assert _capi.PlanInfo(n_tiles=3, n_planes=13).as_dict()["n_tiles"] == 3 and list(_capi.PlanInfo().as_dict()) == [n for n, _ in _capi.PlanInfo._fields_]
    o = _capi.make_options(host_only=1)
    assert (o.struct_size, o.abi_version, o.device, o.host_only) == (C.sizeof(_capi.Options), _capi.ABI_VERSION, -1, 1)
    assert _capi.ABI_VERSION == _capi.TSAMD_ABI_VERSION and _capi.TSAMD_SMOOTH_TAUBIN == 0 and _capi.TSAMD_ERR_HOST_ONLY == 7
    assert set(_capi.SIGNATURES) == set(_capi.HEADER.functions)
    # *_dev fields take plain integers, the tile view's host pointers can be indexed
    assert all(t is C.c_void_p for n, t in _capi.BlendPlanStruct._fields_ + _capi.SmoothMeshStruct._fields_ if n.endswith("_dev"))
    assert dict(_capi.TileView._fields_)["planes"] is P(C.c_uint32) and dict(_capi.TileView._fields_)["row_start"] is P(C.c_uint16)


def test_every_constant_of_the_header_by_name():
    """The names and values by this test's own regexes (not the reader's): every integer #define and every member of the enum."""
    text = _without_comments(_header_text())
    want = {n: int(v) for n, v in re.findall(r"^#define (TSAMD_\w+) (-?\d+)\s*$", text, re.M)}
    enum = re.search(r"typedef enum tsamd_status \{(.*?)\}", text, re.S).group(1)
    want.update({n: int(v) for n, v in re.findall(r"(TSAMD_\w+) = (\d+)", enum)})
    assert len(want) > 40 and want == _capi.HEADER.constants
    for name, value in want.items():
        assert getattr(_capi, name) == value and type(getattr(_capi, name)) is int


def test_constant_maps_of_the_modules_are_the_headers():
    from tssplat_amd import dr, merge, metrics, network, quality, simplify, smooth, voxelize
    assert smooth.MODES == {"taubin": 0, "tangential": 1} and smooth.BOUNDARIES == {"fixed": 0, "free": 1}
    assert merge.FILL_MODES == {"cavities": 1, "outer": 2} and (metrics._SAMPLE_WEIGHTS, metrics._SAMPLE_DRAW) == (0, 1)
    assert voxelize.RULES == {"nonzero": 0, "positive": 1, "odd": 2} and simplify.PLACEMENTS == {"quadric": 0, "mean": 1}
    assert quality._STATS == ("crossing_pairs", "crossing_faces", "invalid_faces", "degenerate_faces", "box_pairs", "listed_pairs", "tile_visits")
    assert network.ACTIVATIONS == {"relu": 1, "none": 0}
    assert dr._TEX_FILTERS == {"nearest": 0, "linear": 1} and dr._TEX_BOUNDARIES == {"wrap": 0, "clamp": 1, "zero": 2}


def test_exceptions_name_declared_parameters_and_differ_from_the_rule():
    """An exception that names nothing, or that the rule would give anyway, has become unnecessary and fails here."""
    for (function, parameter), kept in _capi.EXCEPTIONS.items():
        assert function in _capi.HEADER.functions, function
        ruled = dict(_capi.HEADER.functions[function][1])
        assert parameter in ruled, (function, parameter)
        assert ruled[parameter] is not kept, (function, parameter, kept)
        names = [p for p, _ in _capi.HEADER.functions[function][1]]
        assert _capi.SIGNATURES[function][1][names.index(parameter)] is kept
    # everywhere else SIGNATURES is the rule's reading, argument for argument
    for name, (restype, params) in _capi.HEADER.functions.items():
        assert _capi.SIGNATURES[name][0] is restype and len(_capi.SIGNATURES[name][1]) == len(params)
        for (p, t), got in zip(params, _capi.SIGNATURES[name][1]):
            assert got is _capi.EXCEPTIONS.get((name, p), t), (name, p)


def test_rule_on_the_real_header():
    """Rule R, one parameter of each kind, spelled out against the header's own text."""
    f = {name: dict(params) for name, (_, params) in _capi.HEADER.functions.items()}
    assert f["tsamd_create"] == {"rest_xyz": C.c_void_p, "n_vertices": C.c_int64, "tets": C.c_void_p, "n_tets": C.c_int64,
                                 "options": P(_capi.Options), "out": P(C.c_void_p)}
    assert f["tsamd_create_from_veg"]["path"] is C.c_char_p and f["tsamd_get_tile"]["out"] is P(_capi.TileView)
    assert f["tsamd_get_finish_lists"] == {"h": C.c_void_p, "n_finish": P(C.c_int64), "vid": P(P(C.c_int32)), "off": P(P(C.c_int32)), "idx": P(P(C.c_int32))}
    assert f["tsamd_read_energy_terms"] == {"h": C.c_void_p, "stream": C.c_void_p, "terms_host2": P(C.c_double)}
    assert f["tsamd_sample_surface"]["seed"] is C.c_uint64 and f["tsamd_sample_surface"]["phase"] is C.c_int32
    assert f["tsamd_smooth_run"]["result_in_b_out"] is P(C.c_int32) and f["tsamd_smooth_run"]["mesh"] is P(_capi.SmoothMeshStruct)
    assert f["tsamd_smooth_run"]["lam"] is C.c_double and f["tsamd_smooth_run"]["state_a_dev"] is C.c_void_p
    assert _capi.HEADER.functions["tsamd_last_error"] == (C.c_char_p, []) and _capi.HEADER.functions["tsamd_destroy"][0] is None
    assert _capi.HEADER.functions["tsamd_num_tets"][0] is C.c_int64 and _capi.HEADER.functions["tsamd_abi_version"][0] is C.c_int32


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_c_compiler_reads_the_header_as_we_do(tmp_path):
    """The independent witness: a C program that includes the header prints sizeof, and offsetof / sizeof of every field, of the six
    structs and the value of every TSAMD_* enum member and integer #define; the ctypes classes and the constants must say the same.
    The struct and constant names, and the number of fields per struct, come from this test's own reading of the text."""
    text = _without_comments(_header_text())
    bodies = dict((name, body) for body, name in re.findall(r"typedef struct \w+ \{(.*?)\}\s*(\w+);", text, re.S))
    assert set(bodies) == set(STRUCTS)
    constants = re.findall(r"^#define (TSAMD_\w+) \S", text, re.M) + re.findall(r"^\s*(TSAMD_\w+) = ", text, re.M)
    assert sorted(constants) == sorted(_capi.HEADER.constants)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tssplat_amd.h"', "int main(void) {"]
    for name, cls in STRUCTS.items():
        assert len(cls._fields_) == bodies[name].count(",") + bodies[name].count(";"), name        # one field per declarator
        lines.append(f'    printf("{name} . %zu %zu\\n", (size_t)0, sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f, _ in cls._fields_]
    lines += [f'    printf("constant {c} 0 %lld\\n", (long long)({c}));' for c in constants]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    built = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(_build.HEADER), str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    seen = {(owner, name): (int(a), int(b)) for owner, name, a, b in (ln.split() for ln in out.splitlines())}
    ours = {("constant", c): (0, v) for c, v in _capi.HEADER.constants.items()}
    for name, cls in STRUCTS.items():
        ours[(name, ".")] = (0, C.sizeof(cls))
        ours.update({(name, f): (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_})
    assert seen == ours, {k: (seen.get(k), ours.get(k)) for k in set(seen) | set(ours) if seen.get(k) != ours.get(k)}
