"""CPU: the C headers are the contract, and the Python side is held to them in one place.  The reader (cheader.py) finds every prototype and
struct of include/shc_batch.h and oracle/shc_oracle.h; every struct has a ctypes mirror whose members the host C compiler judges - size of the
struct, offset and size of every member, names in order; the field-name tuples of the four row passes are the enums' own order; and the reader
refuses a construct it does not know.  Nothing here needs a device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from syropod_highlevel_controller_amd import cheader, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {"shc_": os.path.join(ROOT, "include", "shc_batch.h"), "orc_": os.path.join(ROOT, "oracle", "shc_oracle.h")}
ROW_PASS_PREFIX = {"observation": "SHC_OBS_", "action": "SHC_ACT_", "foothold": "SHC_FH_", "reach": "SHC_REACH_"}


def _identifier_before(text: str) -> str:
    end = len(text.rstrip())
    start = end
    while start > 0 and (text[start - 1].isalnum() or text[start - 1] == "_"):
        start -= 1
    return text[start:end]


@pytest.mark.parametrize("prefix, n_functions, n_structs", [("shc_", 157, 20), ("orc_", 91, 0)])
def test_the_reader_misses_no_prototype_and_no_struct(prefix, n_functions, n_structs):
    """An independent crude count on the comment-stripped text: every identifier with the library's prefix that is followed by '(' is a
    function of the reader's (the opaque handle types are no calls), and every `typedef struct X {` is one of its structs."""
    header = cheader.read(PATHS[prefix])
    chunks = cheader.strip_comments(open(PATHS[prefix]).read()).split("(")
    called = {_identifier_before(c) for c in chunks[:-1]}
    assert {c for c in called if c.startswith(prefix)} - set(header.opaque) == set(header.functions)
    bodies = {c.split()[0] for c in cheader.strip_comments(open(PATHS[prefix]).read()).split("typedef struct ")[1:] if c.split()[1] == "{"}
    assert bodies == set(header.structs)
    assert (len(header.functions), len(header.structs)) == (n_functions, n_structs)


def test_the_reader_understands_the_c_the_headers_use():
    h = cheader.parse('''#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define X_N 3 /* three */
enum { X_A, X_B = 1 << 4, X_C, X_D = X_N, X_E = -2, X_F = 0x10 };
typedef struct x_in { double min, max; int32_t n, v[X_N]; double m[X_N][2]; const double *p, *q; } x_in;
typedef struct x_h x_h; /* opaque */
struct x_later;
int x_f(x_h *h /* the handle */, const double quat[4], void *const *dst,
        const struct x_later *l);
const char *x_name(void);
void x_g(const x_in *in, x_h **out);
#ifdef __cplusplus
}
#endif
#endif
''')
    assert h.constants == {"X_N": 3, "X_A": 0, "X_B": 16, "X_C": 17, "X_D": 3, "X_E": -2, "X_F": 16}
    assert h.enums == (("X_A", "X_B", "X_C", "X_D", "X_E", "X_F"),) and h.enum_of("X_C") == h.enums[0]
    assert h.structs == {"x_in": [("double", "min", ()), ("double", "max", ()), ("int32_t", "n", ()), ("int32_t", "v", (3,)), ("double", "m", (3, 2)),
                                  ("const double *", "p", ()), ("const double *", "q", ())]}
    assert h.opaque == ("x_h",)
    assert h.functions == {"x_f": ("int", [("x_h *", "h"), ("const double [4]", "quat"), ("void *const *", "dst"), ("const struct x_later *", "l")]),
                           "x_name": ("const char *", []), "x_g": ("void", [("const x_in *", "in"), ("x_h **", "out")])}
    assert [cheader.ctype(t) for t, _ in h.functions["x_f"][1]] == [C.c_void_p] * 4
    assert cheader.ctype("const char *", returned=True) is C.c_char_p and cheader.ctype("void", returned=True) is None
    assert cheader.ctype("x_h *", returned=True) is C.c_void_p and cheader.ctype("size_t", returned=True) is C.c_size_t


@pytest.mark.parametrize("line", ["union x_u { int a; };", "#if X_N > 2", "static inline int x_f(void) { return 1; }", "int x_f(int);",
                                  "#define X_MAX(a, b) ((a) > (b) ? (a) : (b))", "enum { X_A = 1 + 2 };", "typedef int x_t;"])
def test_the_reader_refuses_what_it_does_not_understand(line):
    with pytest.raises(cheader.HeaderError, match=r"^x\.h:2: "):
        cheader.parse("int x_a(void);\n" + line + "\nint x_b(void);\n", "x.h")


def test_the_binding_gives_the_timed_calls_their_classes():
    """What bench.py calls inside its timed regions takes the engine handle and scalars: these classes are what they have always been."""
    lib = engine.lib()
    assert engine.EXPORTED_SYMBOLS == list(cheader.read(PATHS["shc_"]).functions)
    for name, argtypes in (("shc_engine_resident_publish", [C.c_void_p, C.c_int64]), ("shc_engine_step", [C.c_void_p, C.c_int]),
                           ("shc_engine_set_tip_force", [C.c_void_p, C.c_void_p, C.c_int])):
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is C.c_int, name
    assert lib.shc_last_error.restype is C.c_char_p and lib.shc_engine_instances.restype is C.c_int64


def _host_c_compiler():
    for cmd in (["gcc"], ["cc"], ["clang"], [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c"]):
        if shutil.which(cmd[0]):
            return cmd
    raise FileNotFoundError("no host C compiler (gcc, cc, clang or hipcc)")


def test_every_struct_has_a_mirror_the_c_compiler_agrees_with(tmp_path):
    """Names and their order by comparison; sizeof the struct, offsetof and sizeof every member by _Static_assert in one C file that includes the
    header: compiled to an object, never run."""
    structs = cheader.read(PATHS["shc_"]).structs
    assert set(structs) == set(engine.STRUCT_MIRRORS), set(structs) ^ set(engine.STRUCT_MIRRORS)
    lines = ["#include <stddef.h>", '#include "shc_batch.h"']
    for name, fields in structs.items():
        mirror = engine.STRUCT_MIRRORS[name]
        assert [f for f, _ in mirror._fields_] == [f for _, f, _ in fields], name
        lines.append(f'_Static_assert(sizeof({name}) == {C.sizeof(mirror)}, "sizeof({name})");')
        for f, typ in mirror._fields_:
            lines.append(f'_Static_assert(offsetof({name}, {f}) == {getattr(mirror, f).offset}, "offsetof({name}, {f})");')
            lines.append(f'_Static_assert(sizeof((({name} *)0)->{f}) == {C.sizeof(typ)}, "sizeof {name}.{f}");')
    src = tmp_path / "mirrors.c"
    src.write_text("\n".join(lines) + "\n")
    cmd = _host_c_compiler() + ["-std=c11", "-I", os.path.dirname(PATHS["shc_"]), "-c", "-o", str(tmp_path / "mirrors.o"), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, f"{' '.join(cmd)}\n{built.stderr[-4000:]}"


@pytest.mark.parametrize("kind", sorted(ROW_PASS_PREFIX))
def test_the_field_name_tuples_are_the_enums(kind):
    header, p, prefix = cheader.read(PATHS["shc_"]), engine._ROW_PASSES[kind], ROW_PASS_PREFIX[kind]
    for i, name in enumerate(p.names):
        assert header.constants[prefix + name.upper()] == i and p.index[name] == i, name
    assert header.constants[prefix + "FIELD_COUNT"] == len(p.names)
    assert header.enum_of(prefix + "FIELD_COUNT") == tuple(prefix + name.upper() for name in p.names) + (prefix + "FIELD_COUNT",)
    (dims,) = [d for _, f, d in header.structs[{v: k for k, v in engine.STRUCT_MIRRORS.items()}[p.struct]] if f == "fields"]
    assert (dict(p.struct._fields_)["fields"]._length_,) == dims
