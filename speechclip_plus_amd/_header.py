"""Strict reader of include/speechclip_hip.h: the ctypes binding (``_lib.py``) is derived from the header every C source compiles
against, not typed a second time.  It understands exactly the C that header uses - comments, ``#ifndef`` / ``#ifdef`` / ``#endif`` /
``#include`` / ``#define NAME [integer]``, one ``extern "C" { }`` pair, ``typedef scalar name;``, ``typedef struct { ... } name;`` and
prototypes - and raises ``HeaderError`` quoting the text on anything else: no declaration is ever skipped.  Standard library only."""
import collections
import ctypes
import re

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "uint16_t": ctypes.c_uint16, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float,
           "double": ctypes.c_double}

# defines: NAME -> int;  structs: C name -> ctypes.Structure class;  functions: name -> (restype, [argtypes]), in header order
Header = collections.namedtuple("Header", "defines structs functions")

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DIRECTIVE = re.compile(r"#\s*(ifndef|ifdef|endif|include|define)\b\s*(.*)")
_DEFINE = re.compile(r"(\w+)(?:\s+(\S+))?")
_SPACE = re.compile(r"\s*")
_EXTERN = re.compile(r'extern\s*"C"\s*\{')
_CLOSE = re.compile(r"\}\s*\Z")
_ALIAS = re.compile(r"typedef\s+(\w+)\s+(\w+)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"(const\s+char\s*\*\s*|\w+\s+)(\w+)\s*\(([^(){};]*)\)\s*;")
_DECL = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)        # [const] T, then the declarators
_DECLARATOR = re.compile(r"(\*?)\s*([A-Za-z_]\w*)")              # [*] name: one pointer level, no arrays, no bit-fields


class HeaderError(ValueError):
    pass


def parse(text: str, struct_names=None) -> Header:
    """``struct_names``: C struct name -> name of the ctypes class made for it (default: the C name)."""
    defines, structs, functions, scalars = {}, {}, {}, dict(SCALARS)

    def declarators(decl, where):
        """'const T *p, *q' -> [(p, ctype), (q, ctype)]"""
        decl = decl.strip()
        m = _DECL.fullmatch(decl)
        parts = [_DECLARATOR.fullmatch(d.strip()) for d in m.group(2).split(",")] if m else [None]
        if not all(parts):
            raise HeaderError(f"cannot parse the declaration {decl!r} in {where!r}")
        base, out = m.group(1), []
        for star, name in (p.groups() for p in parts):
            if not star and base in scalars:
                t = scalars[base]
            elif star and base in structs:
                t = ctypes.POINTER(structs[base])
            elif star and base in scalars:       # the header's convention: *_host is a HOST array of scalars, every other pointer a device address
                t = ctypes.POINTER(scalars[base]) if name.endswith("_host") else ctypes.c_void_p
            elif star and base == "void" and not name.endswith("_host"):
                t = ctypes.c_void_p
            else:
                raise HeaderError(f"unknown type {base!r} in the declaration {decl!r} in {where!r}")
            out.append((name, t))
        return out

    lines = []
    for line in _COMMENT.sub(" ", text).split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            lines.append(line)
            continue
        m = _DIRECTIVE.fullmatch(s)
        d = _DEFINE.fullmatch(m.group(2)) if m and m.group(1) == "define" else None
        if not m or s.endswith("\\") or (m.group(1) == "define" and not d):
            raise HeaderError(f"unsupported preprocessor line {s!r}")
        if d and d.group(2) is not None:
            try:
                defines[d.group(1)] = int(d.group(2), 0)
            except ValueError:
                raise HeaderError(f"#define with a value that is no integer: {s!r}") from None
    text, pos, in_extern = "\n".join(lines), 0, False
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        if not in_extern and (m := _EXTERN.match(text, pos)):
            in_extern = True
        elif in_extern and (m := _CLOSE.match(text, pos)):                      # the closing brace of extern "C": the last thing
            in_extern = False
        elif m := _ALIAS.match(text, pos):
            if m.group(1) not in scalars:
                raise HeaderError(f"unknown type {m.group(1)!r} in {m.group(0)!r}")
            scalars[m.group(2)] = scalars[m.group(1)]
        elif m := _STRUCT.match(text, pos):
            body, cname = m.groups()
            *stmts, rest = body.split(";")
            if rest.strip() or cname in structs:
                raise HeaderError(f"cannot parse {rest.strip()!r} at the end of struct {cname}, or its second declaration")
            fields = [f for s in stmts for f in declarators(s, "struct " + cname)]
            structs[cname] = type((struct_names or {}).get(cname, cname), (ctypes.Structure,), {"_fields_": fields})
        elif m := _PROTO.match(text, pos):
            ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
            where = " ".join(m.group(0).split())
            restype = ctypes.c_char_p if "".join(ret.split()) == "constchar*" else scalars.get(ret)
            if restype is None:
                raise HeaderError(f"unknown return type {ret!r} in {where!r}")
            if not args or name in functions:
                raise HeaderError(f"empty argument list (write (void)) or second declaration: {where!r}")
            functions[name] = (restype, [] if args == "void" else [declarators(a, where)[0][1] for a in args.split(",")])
        else:
            end = text.find(";", pos)
            raise HeaderError(f"cannot parse {' '.join(text[pos:end + 1 if end >= 0 else len(text)].split())[:400]!r}")
        pos = m.end()
    if in_extern:
        raise HeaderError('extern "C" { is never closed')
    return Header(defines, structs, functions)


def read(path: str, struct_names=None) -> Header:
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise RuntimeError(f"{path}: the C header the ctypes binding is derived from cannot be read ({e})") from None
    return parse(text, struct_names)
