"""CPU: the binding is derived from include/dqo_raster.h by dqo-map_amd/_dqo_header.py, and two things hold the reader in place.

The layout — a C program that includes the header and prints sizeof of every struct and offsetof / sizeof of every field, generated from
the header's text by this file's own regexes (not by the reader) and compiled by the host C compiler as C99, must agree with every
binding class: the same structs, the same size, the same field names in the same order at the same offsets.  The refusals — the reader
never guesses: an unknown type, a declarator it cannot split, a `dqo_x(` it did not parse and a constant expression outside its grammar
each raise and name the line; a well-formed header gives exactly the expected lists."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dqo_raster.h")


@pytest.fixture(scope="module")
def native():
    import _dqo_native
    return _dqo_native


@pytest.fixture(scope="module")
def reader():
    import _dqo_header
    return _dqo_header


def _declared_structs():
    """[(struct, [field, ...])] by this test's own reading of the header"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = []
    for name, body in re.findall(r"typedef struct (Dqo\w+) \{(.*?)\} \1;", src, flags=re.S):
        out.append((name, re.findall(r"[*\s](\w+)(?:\[\d+\])?(?=[,;])", body)))
    return out


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """{struct: (sizeof, [(field, offsetof, sizeof), ...])} as the host C compiler lays the header out"""
    cc = shutil.which("cc")
    assert cc, "no host C compiler (cc): the layout of the binding cannot be checked"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for name, fields in _declared_structs():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        for f in fields:
            lines.append(f'    printf("F {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
    lines += ["    return 0;", "}", ""]
    d = tmp_path_factory.mktemp("layout")
    (d / "layout.c").write_text("\n".join(lines))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-o", str(d / "layout"), str(d / "layout.c")], check=True)
    out = {}
    for line in subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        if w[0] == "S":
            out[w[1]] = (int(w[2]), [])
        else:
            out[w[1]][1].append((w[2], int(w[3]), int(w[4])))
    return out


def test_every_binding_class_has_the_compilers_layout(native, compiled_layout):
    classes = {k: v for k, v in vars(native).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    assert sorted(classes) == sorted(compiled_layout) and len(classes) >= 18
    assert sum(len(f) for _, f in compiled_layout.values()) >= 261
    for name, (size, fields) in compiled_layout.items():
        cls = classes[name]
        assert ctypes.sizeof(cls) == size, name
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields], name
        for n, offset, width in fields:
            assert (getattr(cls, n).offset, getattr(cls, n).size) == (offset, width), (name, n)
    assert set(native.ABI_SIZEOF_ORDER) - {None} == set(classes)  # every struct has its index in dqo_abi_sizeof


def test_the_module_constants_are_the_headers(native):
    c = native.CONSTANTS
    assert (native.ROW_FROZEN, native.ROW_HIDDEN, native.TICKET_WORDS) == (c["DQO_ROW_FROZEN"], c["DQO_ROW_HIDDEN"], c["DQO_TICKET_WORDS"])
    assert (native.ROW_FROZEN, native.ROW_HIDDEN, native.TICKET_WORDS, c["DQO_ABI_VERSION"]) == (1, 2, 16 + 16 * 64, 5)
    assert native.WINDOW_BANK_STATE_WORDS == c["DQO_WINDOW_BANK_STATE_WORDS"] == native.TICKET_WORDS + 48
    assert native.WINDOW_BANK_WORDS == ("cursor", "n", "prev_k", "prev_m", "force", "overrun", "lost_count")
    assert [c["DQO_WINDOW_BANK_" + w.upper()] - native.TICKET_WORDS for w in native.WINDOW_BANK_WORDS] == list(range(7))
    assert native.REPOSE_TARGET_FIELDS == ("row", "c2w", "w2c", "viewmatrix", "projmatrix", "campos") and native.REPOSE_HAS_PROJMATRIX == 1
    assert (c["DQO_OK"], c["DQO_ERR_OVERFLOW"], c["DQO_ATE_MAX_POINTS"], c["DQO_TRAJ_LISTED"]) == (0, -4, 1 << 24, 4)
    assert native.EXPORTS == tuple(native.PROTOTYPES) and len(native.EXPORTS) >= 129


MINI = """/* a header in the dialect of dqo_raster.h; dqo_not_code(1) in a comment is no prototype */
#ifndef MINI_H_
#define MINI_H_
#include <stdint.h>
#define DQO_A 3u /* DQO_IGNORED 7 */
#define DQO_B (DQO_A + 2 * (1 << 4))
typedef enum DqoE { DQO_E0 = 0, DQO_E1 = -1, DQO_E2 } DqoE;
enum { DQO_F = DQO_B - 1 };
typedef struct DqoMini {
    int32_t W, H;        /* two fields */
    const float* a;      // a pointer
    float *m, *v;
    char name[8];
    double d; uint8_t u;
    size_t n;
    const DqoOther* other;
} DqoMini;
int dqo_version(void);
const char* dqo_error(void);
size_t dqo_bytes(int32_t n, int64_t cap);
int64_t dqo_count(const DqoMini*, DqoMini* out, const float* x, float f, double d,
                  uint64_t seed, uint32_t k, int flag, void* stream);
#endif
"""


def test_a_well_formed_header_gives_exactly_these_lists(reader):
    c = ctypes
    h = reader.parse(MINI)
    assert h.constants == {"DQO_A": 3, "DQO_B": 35, "DQO_E0": 0, "DQO_E1": -1, "DQO_E2": 0, "DQO_F": 34}
    assert list(h.structs) == ["DqoMini"]
    fields = h.structs["DqoMini"]
    assert [n for n, _ in fields] == ["W", "H", "a", "m", "v", "name", "d", "u", "n", "other"]
    assert [t for _, t in fields[:5]] + [t for _, t in fields[6:]] == [c.c_int32, c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_double,
                                                                       c.c_uint8, c.c_size_t, c.c_void_p]
    assert fields[5][1]._type_ is c.c_char and fields[5][1]._length_ == 8
    assert list(h.functions) == ["dqo_version", "dqo_error", "dqo_bytes", "dqo_count"]
    assert h.functions["dqo_version"] == (c.c_int, []) and h.functions["dqo_error"] == (c.c_char_p, [])
    assert h.functions["dqo_bytes"] == (c.c_size_t, [c.c_int32, c.c_int64])
    assert h.functions["dqo_count"] == (c.c_int64, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_float, c.c_double, c.c_uint64, c.c_uint32, c.c_int,
                                                    c.c_void_p])


REFUSED = [
    ("unknown field type", "typedef struct DqoX {\n    int32_t a;\n    long b;\n} DqoX;\n", 3, "unknown type 'long'"),
    ("unknown parameter type", "\n\nint dqo_f(int32_t a, unsigned b);\n", 3, "unknown type 'unsigned'"),
    ("unknown return type", "float dqo_f(int32_t a);\n", 1, "unknown return type 'float'"),
    ("struct by value", "int dqo_f(DqoX x);\n", 1, "unknown type 'DqoX'"),
    ("star on one name only", "typedef struct DqoX {\n    float *a, b;\n} DqoX;\n", 2, "cannot split declarator"),
    ("pointer to pointer", "int dqo_f(float** a);\n", 1, "cannot split declarator"),
    ("array parameter", "int dqo_f(float a[4]);\n", 1, "cannot split declarator"),
    ("unparsed dqo_x(", "int dqo_ok(void);\n#define CALL(x) dqo_hidden(x)\n", 2, "dqo_hidden"),
    ("prototype not at column 0", "int dqo_ok(void);\n  int dqo_indented(void);\n", 2, "dqo_indented"),
    ("function pointer parameter", "int dqo_f(void (*cb)(int), void* s);\n", 1, "dqo_f"),
    ("division in a constant", "#define DQO_A 4\n#define DQO_B (DQO_A / 2)\n", 2, "constant expression"),
    ("hexadecimal constant", "#define DQO_A 0x10\n", 1, "constant expression"),
    ("later constant", "enum { DQO_A = DQO_B + 1, DQO_B = 2 };\n", 1, "'DQO_B'"),
    ("unbalanced constant", "#define DQO_A (1 + 2\n", 1, "does not evaluate"),
    ("sizeof in an enumerator", "enum {\n    DQO_A = sizeof(int)\n};\n", 2, "constant expression"),
]


@pytest.mark.parametrize("text,line,message", [r[1:] for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_the_reader_refuses_and_names_the_line(reader, text, line, message):
    with pytest.raises(ValueError, match=rf"mini\.h:{line}: .*{re.escape(message)}"):
        reader.parse(text, "mini.h")


def test_a_missing_header_is_named(reader, tmp_path):
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "dqo_raster.h"))):
        reader.load(str(tmp_path / "dqo_raster.h"))
    assert reader.HEADER_PATH == HEADER
