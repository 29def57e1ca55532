"""Reader of the project's C headers: prototypes, struct bodies and integer constants, and the one rule that turns a prototype into ctypes
classes.  Standard library only.  It takes a path and knows no library: the product's binding and the tests' oracle binding both use it.

It understands the C those headers are written in and nothing more - block and line comments anywhere, ``#define NAME <integer>``, include
guards, ``#include``, the ``extern "C"`` guard, ``enum { ... };``, ``typedef struct X { ... } X;``, opaque ``typedef struct X X;``, forward
``struct X;`` and prototypes.  Anything else at the top level raises HeaderError with the header's line; nothing is skipped.
"""
from __future__ import annotations

import ctypes as C
import functools
import re
from typing import NamedTuple


class HeaderError(ValueError):
    pass


class Header(NamedTuple):
    functions: dict   # {name: (return type, [(type text, parameter name)])}, in the header's order
    structs: dict     # {name: [(type, field name, dims)]} of every struct with a body; dims = () or the array lengths as integers
    opaque: tuple     # names of the opaque typedefs (typedef struct X X;)
    constants: dict   # {name: int} of every #define NAME <integer> and every enumerator
    enums: tuple      # one tuple of enumerator names per enum { ... } block, in order

    def enum_of(self, name: str) -> tuple:
        """The enumerators, in order, of the enum block that declares ``name``."""
        return next(block for block in self.enums if name in block)


_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_TOKEN = re.compile(r"[A-Za-z_]\w*|\*|\[[^\]]*\]")
_IGNORED_DIRECTIVE = re.compile(r"#\s*(ifndef\s+\w+|ifdef\s+__cplusplus|endif|include\s*[<\"][^>\"]+[>\"]|define\s+\w+)\s*$")
_DEFINE = re.compile(r"#\s*define\s+(\w+)\s+(\S.*?)\s*$")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)$", re.S)
_OPAQUE = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)$")
_FORWARD = re.compile(r"struct\s+\w+$")
_ENUM = re.compile(r"enum\s*\{(.*)\}$", re.S)
_PROTOTYPE = re.compile(r"([\w\s\*]+?)\b(\w+)\s*\((.*)\)$", re.S)


def _type_text(tokens) -> str:
    """'const', 'double', '*' -> 'const double *'; 'void', '*', 'const', '*' -> 'void *const *'."""
    out = ""
    for t in tokens:
        out += t if t == "*" and out.endswith("*") else (t if out.endswith("*") else " " + t)
    return out.strip()


def _value(expr: str, constants: dict, where: str) -> int:
    """An integer literal, an earlier constant, or ``a << b`` of those."""
    def atom(s):
        s = s.strip()
        if s in constants:
            return constants[s]
        try:
            return int(s, 0)
        except ValueError:
            raise HeaderError(f"{where}: {expr.strip()!r} is not an integer constant expression this reader knows") from None
    left, shift, right = expr.partition("<<")
    return atom(left) << atom(right) if shift else atom(left)


def _declarator(tokens, where):
    """(stars, name, dims) of the tail of a declaration: `* name [A] [B]`."""
    dims = []
    while tokens and tokens[-1].startswith("["):
        dims.insert(0, tokens.pop()[1:-1])
    if not tokens or tokens[-1] == "*":
        raise HeaderError(f"{where}: a declaration without a name")
    name = tokens.pop()
    stars = 0
    while tokens and tokens[-1] == "*":
        tokens.pop()
        stars += 1
    return stars, name, dims


def _fields(body: str, constants: dict, where: str):
    out = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        first, *more = decl.split(",")
        tokens = _TOKEN.findall(first)
        stars, name, dims = _declarator(tokens, where)
        if not tokens or "".join(_TOKEN.findall(decl)) != re.sub(r"[\s,]", "", decl):
            raise HeaderError(f"{where}: cannot read the member declaration {' '.join(decl.split())!r}")
        base = _type_text(tokens)
        for stars, name, dims in [(stars, name, dims)] + [_declarator(_TOKEN.findall(d), where) for d in more]:
            out.append((_type_text([base] + ["*"] * stars), name, tuple(_value(d, constants, where) for d in dims)))
    return out


def _parameters(text: str, where: str):
    if text.strip() == "void":
        return []
    out = []
    for p in text.split(","):
        tokens = _TOKEN.findall(p)
        if "".join(tokens) != re.sub(r"\s", "", p):
            raise HeaderError(f"{where}: cannot read the parameter {' '.join(p.split())!r}")
        stars, name, dims = _declarator(tokens, where)
        if not tokens:
            raise HeaderError(f"{where}: the parameter {' '.join(p.split())!r} has no name")
        out.append((_type_text(tokens + ["*"] * stars + [f"[{d}]" for d in dims]), name))
    return out


def strip_comments(text: str) -> str:
    """The text with every comment blanked out: line numbers stay."""
    return _COMMENT.sub(lambda m: re.sub(r"[^\n]", " ", m.group(0)), text)


def parse(text: str, origin: str = "<header>") -> Header:
    """Read header text; ``origin`` names it in errors."""
    functions, structs, opaque, constants, enums = {}, {}, [], {}, []
    text = strip_comments(text)
    pos, extern_c = 0, False
    while True:
        while pos < len(text) and text[pos].isspace():
            pos += 1
        if pos == len(text):
            break
        where = f"{origin}:{text.count(chr(10), 0, pos) + 1}"
        if text[pos] == "#":
            end = text.find("\n", pos)
            end = len(text) if end < 0 else end
            line = text[pos:end]
            m = _DEFINE.match(line)
            if m:
                constants[m.group(1)] = _value(m.group(2), constants, where)
            elif not _IGNORED_DIRECTIVE.match(line.rstrip()):
                raise HeaderError(f"{where}: unknown preprocessor line {line.strip()!r}")
            pos = end
            continue
        if text.startswith('extern "C" {', pos) and not extern_c:
            extern_c, pos = True, pos + len('extern "C" {')
            continue
        if text[pos] == "}" and extern_c:
            extern_c, pos = False, pos + 1
            continue
        end, depth = pos, 0   # one statement: up to the ';' outside braces (a preprocessor line never sits inside one in these headers)
        while end < len(text) and (text[end] != ";" or depth):
            depth += {"{": 1, "}": -1}.get(text[end], 0)
            end += 1
        stmt = text[pos:end].strip()
        if end == len(text) or depth or "#" in stmt:
            raise HeaderError(f"{where}: unterminated or unknown construct {' '.join(stmt.split())[:60]!r}")
        pos = end + 1
        m = _ENUM.match(stmt)
        if m:
            names, nxt = [], 0
            for item in m.group(1).split(","):
                if not item.strip():
                    continue
                name, eq, expr = (s.strip() for s in item.partition("="))
                if not re.fullmatch(r"[A-Za-z_]\w*", name) or name in constants:
                    raise HeaderError(f"{where}: cannot read the enumerator {item.strip()!r}")
                constants[name] = nxt = _value(expr, constants, where) if eq else nxt
                nxt += 1
                names.append(name)
            enums.append(tuple(names))
            continue
        m = _STRUCT.match(stmt)
        if m:
            if m.group(1) != m.group(3) or m.group(1) in structs:
                raise HeaderError(f"{where}: struct {m.group(1)} is typedef'd as {m.group(3)}, or defined twice")
            structs[m.group(1)] = _fields(m.group(2), constants, where)
            continue
        m = _OPAQUE.match(stmt)
        if m and m.group(1) == m.group(2):
            opaque.append(m.group(1))
            continue
        if _FORWARD.match(stmt):
            continue
        m = _PROTOTYPE.match(stmt)
        if m and "{" not in stmt and "=" not in stmt and not stmt.startswith("typedef"):
            ret, name, params = m.groups()
            if name in functions:
                raise HeaderError(f"{where}: {name} is declared twice")
            functions[name] = (_type_text(_TOKEN.findall(ret)), _parameters(params, where))
            continue
        raise HeaderError(f"{where}: unknown construct {' '.join(stmt.split())[:60]!r}")
    if extern_c:
        raise HeaderError(f"{origin}: the extern \"C\" block is never closed")
    return Header(functions, structs, tuple(opaque), constants, tuple(enums))


@functools.lru_cache(maxsize=None)
def read(path: str) -> Header:
    """The header at ``path``, read once per process."""
    try:
        with open(path, "r") as f:
            text = f.read()
    except OSError as exc:
        raise ImportError(f"the C header {path} cannot be read ({exc.strerror}): the Python binding takes its signatures and constants from it") from None
    return parse(text, path)


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double, "size_t": C.c_size_t}


def ctype(type_text: str, returned: bool = False):
    """The ctypes class of a parameter or return type: a scalar maps to its class, a returned ``const char *`` to c_char_p, a returned ``void``
    to None, every other pointer (array-typed parameters included) to c_void_p - which takes byref(...), ctypes arrays and pointers, integers
    that are addresses, bytes and None."""
    if "*" in type_text or "[" in type_text:
        return C.c_char_p if returned and type_text == "const char *" else C.c_void_p
    if returned and type_text == "void":
        return None
    try:
        return _SCALARS[type_text]
    except KeyError:
        raise HeaderError(f"no ctypes class for the C type {type_text!r}") from None


def bind(library, functions: dict) -> None:
    """Give every declared function of the loaded ``library`` its restype and argtypes (a missing symbol is an AttributeError)."""
    for name, (ret, params) in functions.items():
        fn = getattr(library, name)
        fn.restype = ctype(ret, returned=True)
        fn.argtypes = [ctype(t) for t, _ in params]
