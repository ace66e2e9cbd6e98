"""Reader of include/dqo_raster.h: the structs, prototypes and integer constants of the C ABI as ctypes, so that the header is the one
place an operator's boundary is written (_dqo_native.py builds itself from this).  Standard library only.

The header is plain C with prototypes at column 0; what is read, after the comments are taken out:
  structs     `typedef struct DqoX { ... } DqoX;`  -> [(field name, ctypes type)], in order; `int32_t W, H;` and `float *m, *v;` declare two fields each
  prototypes  `ret dqo_name(args);`                -> (restype, [argtypes]); parameter names are optional, `(void)` is no argument
  constants   `#define DQO_X <int expr>` and enumerators (named or anonymous enums, an enumerator without a value is its predecessor
              + 1) -> {name: int}.  An expression holds integer literals (a `u` suffix allowed), + - * <<, parentheses and the names of
              earlier constants, nothing else.

Rules of the derivation:
  scalars   by name: int, int32_t, uint32_t, int64_t, uint64_t, size_t, float, double, uint8_t, and `char name[N]` in a struct.
  pointers  every pointer, field or parameter, is c_void_p, whatever it points to and const or not: call sites pass byref(struct),
            integer device addresses, None, ctypes arrays and cast(arr, c_void_p), and c_void_p takes all five.  This gives up
            POINTER(DqoX) type checking of host struct arguments: a struct of the wrong type is not refused by ctypes.
  returns   int -> c_int, size_t -> c_size_t, int64_t -> c_int64, const char* -> c_char_p.
  refusals  never a guess: an unknown type, a declarator that does not split, a `dqo_` identifier followed by `(` that is not a parsed
            prototype, and a constant expression outside the grammar above each raise ValueError naming the line.
"""
import ctypes
import os
import re
from typing import NamedTuple

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dqo_raster.h"))

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
           "uint8_t": ctypes.c_uint8}
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}


class Header(NamedTuple):
    structs: dict    # {"DqoX": [(field, ctype), ...]}
    functions: dict  # {"dqo_name": (restype, [argtype, ...])}, in the header's order
    constants: dict  # {"DQO_X": int}


def _declarator(text, fail):
    """`const T* name`, `T name`, `T` (an unnamed parameter), `T a, b` or `char name[N]` -> (ctype, [names])"""
    text = re.sub(r"\bconst\b", " ", text).strip()
    if "*" in text:  # (`T *a, *b`: every name carries its own star, or the declarator is refused)
        m = re.fullmatch(r"\w+((?:\s*\*\s*\w+\s*,)*\s*\*\s*\w*)", text)
        return (ctypes.c_void_p, re.findall(r"\*\s*(\w*)", m.group(1))) if m else fail(f"cannot split declarator {text!r}")
    m = re.fullmatch(r"char\s+(\w+)\s*\[\s*(\d+)\s*\]", text)
    if m:
        return ctypes.c_char * int(m.group(2)), [m.group(1)]
    m = re.fullmatch(r"(\w+)((?:\s+\w+(?:\s*,\s*\w+)*)?)", text)
    if not m:
        return fail(f"cannot split declarator {text!r}")
    if m.group(1) not in SCALARS:
        return fail(f"unknown type {m.group(1)!r}")
    return SCALARS[m.group(1)], re.findall(r"\w+", m.group(2))


def _constant(expr, known, fail):
    tokens = re.findall(r"\s*(\d+u?\b|DQO_\w+|<<|[-+*()]|.)", expr.strip())
    for i, t in enumerate(tokens):
        if t in known:
            tokens[i] = str(known[t])
        elif re.fullmatch(r"\d+u?", t):
            tokens[i] = t.rstrip("u")
        elif t not in ("<<", "-", "+", "*", "(", ")"):
            return fail(f"constant expression {expr.strip()!r}: {t!r} is neither an integer, + - * <<, a parenthesis nor an earlier constant")
    try:  # (digits, four operators and parentheses only: Python's precedences for them are C's)
        return int(eval(" ".join(tokens), {"__builtins__": {}}))
    except Exception:
        return fail(f"constant expression {expr.strip()!r} does not evaluate")


def parse(text, path="dqo_raster.h"):
    """Header of a header's text (see the module's docstring for the rules)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)  # (keeps the line numbers)

    def failing(pos):
        def fail(msg):
            raise ValueError(f"{path}:{text.count(chr(10), 0, pos) + 1}: {msg}")
        return fail

    constants = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(DQO_\w+)[ \t]+(\S[^\n]*)$|\benum\b[^{;]*\{([^}]*)\}", text, flags=re.M):
        if m.group(1):
            constants[m.group(1)] = _constant(m.group(2), constants, failing(m.start()))
            continue
        value, pos = -1, m.start(3)
        for item in m.group(3).split(","):
            fail = failing(pos + len(item) - len(item.lstrip()))
            e = re.fullmatch(r"\s*(\w+)\s*(?:=(.*))?", item, flags=re.S)
            if e:
                value = value + 1 if e.group(2) is None else _constant(e.group(2), constants, fail)
                constants[e.group(1)] = value
            elif item.strip():
                fail(f"cannot split enumerator {item.strip()!r}")
            pos += len(item) + 1

    structs = {}
    for m in re.finditer(r"\btypedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*(\w+)\s*;", text):
        fields, pos = [], m.start(2)
        for decl in m.group(2).split(";"):
            if decl.strip():
                fail = failing(pos + len(decl) - len(decl.lstrip()))
                ctype, names = _declarator(decl, fail)
                if not names or not all(names):
                    fail(f"cannot split declarator {decl.strip()!r}")
                fields += [(n, ctype) for n in names]
            pos += len(decl) + 1
        if m.group(1) != m.group(3):
            failing(m.start())(f"struct {m.group(1)} is typedef'd as {m.group(3)}")
        structs[m.group(1)] = fields

    functions, parsed = {}, set()
    for m in re.finditer(r"^(\w[\w \t]*?[ \t*]+)(dqo_\w+)[ \t]*\(([^()]*)\)\s*;", text, flags=re.M):
        fail = failing(m.start())
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        if ret not in RETURNS:
            fail(f"unknown return type {ret!r} of {m.group(2)}")
        args = [] if m.group(3).strip() == "void" else [_declarator(a, fail) for a in m.group(3).split(",")]
        functions[m.group(2)] = (RETURNS[ret], [ctype for ctype, _ in args])
        parsed.add(m.start(2))
    for m in re.finditer(r"\bdqo_\w+\s*\(", text):
        if m.start() not in parsed:
            failing(m.start())(f"{m.group().rstrip('( ')} is followed by '(' but is not a prototype this reader parses")
    return Header(structs, functions, constants)


def load(path=HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the binding reads the C ABI from the checkout's include/dqo_raster.h")
    with open(path) as f:
        return parse(f.read(), path)
