"""Reader of include/sfnative.h: the prototypes and integer constants the ctypes binding (_lib.py) is built from.

Strict by design: it knows the vocabulary the header uses today and raises on anything else, so a new kind of prototype fails
at import, named, instead of being bound wrongly.
"""
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sfnative.h")

RETURNS = ("int", "size_t", "const char*")
SCALARS = ("int", "long", "size_t", "float", "double")
POINTEES = ("void", "float", "double", "int32_t", "int64_t", "uint8_t", "uint32_t", "uint64_t", "size_t", "void*")      # + the header's structs

_ARG = re.compile(r"(const )?(\w+) ?(\**) ?\w+ ?(\[\w*\])?")


def parse(text):
    """(prototypes, constants, structs) of a header text: {sf_name: (return type, [argument types])} with the types as C spells
    them ("const float*"; an array argument is a pointer), {SF_NAME: int} for every `#define SF_* <int>` and every enumerator,
    and the names of the typedef'd structs."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {m[1]: int(m[2], 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SF_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern "C" \{(.*)\}', r"\1", text, flags=re.S)      # what is left of the __cplusplus guards
    for m in re.finditer(r"enum\s*\w*\s*\{([^{}]*)\}", text):
        nxt = 0
        for item in filter(None, (s.strip() for s in m[1].split(","))):
            name, _, value = (s.strip() for s in item.partition("="))
            consts[name] = nxt = int(value, 0) if value else nxt
            nxt += 1
    structs = re.findall(r"typedef\s+struct\s+(\w+)\s*\{[^{}]*\}\s*\1\s*;", text)
    text = re.sub(r"(typedef\s+)?(enum|struct)\s*\w*\s*\{[^{}]*\}\s*\w*\s*;", "", text)
    while "{" in text:      # the body of the static inline, innermost braces first
        text, n = re.subn(r"\{[^{}]*\}", "@", text)
        if not n:
            raise ValueError("sfnative.h: unbalanced braces")
    text = re.sub(r"static\s+inline[^;@]*@", "", text)

    protos = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(.*?) ?(sf_\w+) ?\((.*)\)", stmt)
        if not m:
            raise ValueError(f"sfnative.h: not a prototype: {stmt!r}")
        ret, name, args = re.sub(r" ?\* ?", "*", m[1]), m[2], m[3]
        if ret not in RETURNS:
            raise ValueError(f"sfnative.h: {name}: return type {ret!r} is outside the binding's vocabulary")
        types = []
        for arg in ([] if args == "void" else [a.strip() for a in args.split(",")]):
            a = _ARG.fullmatch(arg)
            if not a:
                raise ValueError(f"sfnative.h: {name}: cannot read argument {arg!r}")
            const, base, stars = a[1] or "", a[2], a[3] + ("*" if a[4] else "")
            if stars:
                known = base + stars[1:] in POINTEES or (base in structs and stars == "*")
            else:
                known = base in SCALARS and not const
            if not known:
                raise ValueError(f"sfnative.h: {name}: argument {arg!r} is outside the binding's vocabulary")
            types.append(const + base + stars)
        protos[name] = (ret, types)
    return protos, consts, structs


def read():
    with open(HEADER_PATH, encoding="utf-8") as f:
        return parse(f.read())
