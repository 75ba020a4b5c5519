"""A ctypes binding against the C header it restates, as a C compiler sees that header: measure() parses the header and
compiles and runs ONE generated program; the check_* functions take the binding's pieces as arguments and return findings,
[(where, what), ...], empty when all agrees. tests/test_abi_cpu.py turns them on 3dal_pytorch_amd/_hip.py and on planted faults.

The header is read, comments stripped, in two regular shapes only: `typedef struct ... { ... } dal3_x;` and
`<type> dal3_x(<parameters>);`, plus `#define DAL3_X <integer>` and enumerators `DAL3_X = <integer>`. A declaration that
does not fit raises ValueError: the parse is to be fixed then, not the declaration skipped."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

# structs {c name: [(c type, field, is array)]} and prototypes {name: (c return type, [(c type, parameter)])} from the parse;
# sizes {c name: sizeof}, fields {(c name, field): (offsetof, sizeof)}, constants {DAL3_X: value} from the program's output
Abi = collections.namedtuple("Abi", "structs prototypes sizes fields constants")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}


def declarators(decl):
    """`const float* a` | `double lr, beta1` | `int32_t shape[3]` -> [(c type, name, is array), ...]"""
    head, *more = [" ".join(p.split()) for p in decl.split(",")]
    ctype, _, first = head.rpartition(" ")
    names = [re.fullmatch(r"(\w+)(\[\w+\])?", n) for n in [first] + more]
    if not ctype or not all(names):
        raise ValueError(f"`{decl.strip()}` does not fit the parse")
    return [(ctype, m.group(1), bool(m.group(2))) for m in names]


def measure(header_path, work_dir):
    """the header -> Abi, by one compile and one run in `work_dir`"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(header_path).read(), flags=re.S)
    constants = [a or b for a, b in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DAL3_\w+)[ \t]+-?\d+[ \t]*$|\b(DAL3_\w+)\s*=\s*-?\d+\b",
                                               text, re.M)]
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {m.group(2): [f for d in m.group(1).split(";") if d.strip() for f in declarators(d)]
               for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(dal3_\w+)\s*;", text)}
    prototypes = {}
    for m in re.finditer(r"([^;{}()]*?)\b(dal3_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [f for d in m.group(3).split(",") if d.strip() != "void" for f in declarators(d)]
        prototypes[m.group(2)] = (" ".join(m.group(1).split()), [(t + "*" * arr, p) for t, p, arr in params])   # `size_t off[4]` is a pointer
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.basename(header_path)}"', "int main(void) {"]
    for c, fields in structs.items():
        lines.append(f'printf("S {c} . %zu 0\\n", sizeof({c}));')
        lines += [f'printf("F {c} {f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c}*)0)->{f}));' for _, f, _ in fields]
    lines += [f'printf("K {k} . %lld 0\\n", (long long){k});' for k in constants]
    src, exe = os.path.join(str(work_dir), "abi.c"), os.path.join(str(work_dir), "abi")
    with open(src, "w") as f:
        f.write("\n".join(lines + ["return 0; }", ""]))
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    subprocess.run([cc, "-std=c99", "-I", os.path.dirname(header_path), src, "-o", exe], check=True)
    out = [line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    return Abi(structs, prototypes, {a: int(v) for kind, a, _, v, _ in out if kind == "S"},
               {(a, b): (int(v), int(w)) for kind, a, b, v, w in out if kind == "F"}, {a: int(v) for kind, a, _, v, _ in out if kind == "K"})


def mirrors_of(module):
    """every ctypes.Structure defined in `module` -> {class: the C name its docstring starts with, or None}"""
    return {t: (re.match(r"dal3_\w+", t.__doc__ or "") or [None])[0] for t in vars(module).values()
            if isinstance(t, type) and issubclass(t, C.Structure) and t.__module__ == module.__name__}


def type_mismatch(ctype, t, mirrors):
    """None where the ctypes type `t` is of the C type's class, else what differs. Pointer (any `*`, dal3_stream): c_void_p,
    c_char_p or a POINTER, which is held to its pointee too unless C says void; struct by value: its mirror; scalar: the
    same kind, width and signedness."""
    def kind(s):
        scalar = isinstance(s, type) and issubclass(s, C._SimpleCData) and s._type_ in "iIlLqQfd"
        return scalar and (s._type_ in "fd", s._type_.islower(), C.sizeof(s))
    base = re.sub(r"\bconst\b|\*", "", ctype).strip()
    if "*" in ctype or base == "dal3_stream":
        ok = t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer) and (
            base in ("void", "dal3_stream") or not type_mismatch(base, t._type_, mirrors)))
    else:
        ok = kind(t) == kind(SCALARS[base]) if base in SCALARS else mirrors.get(t) == base
    return None if ok else f"{getattr(t, '__name__', t)} for `{ctype}`"


def check_struct(cname, mirror, abi, mirrors):
    """one ctypes.Structure against the header's struct: sizeof, the fields' names in order, each one's offset, size and type"""
    out = [(cname, f"sizeof {C.sizeof(mirror)}, header {abi.sizes[cname]}")] if C.sizeof(mirror) != abi.sizes[cname] else []
    want, types = [f for _, f, _ in abi.structs[cname]], dict(f[:2] for f in mirror._fields_)
    out += [(f"{cname}.{f}", "not in the mirror") for f in want if f not in types]
    out += [(f"{cname}.{f}", "not in the header") for f in types if f not in want]
    if sorted(want) == sorted(types):
        out += [(f"{cname}.{w}", f"field {i} of the header, the mirror has {g} there") for i, (w, g) in enumerate(zip(want, types)) if w != g]
    for ctype, f, arr in abi.structs[cname]:
        if f in types:
            d, t = getattr(mirror, f), types[f]
            is_arr = isinstance(t, type) and issubclass(t, C.Array)
            bad = [f"(offset, size) {(d.offset, d.size)}, header {abi.fields[cname, f]}"] if (d.offset, d.size) != abi.fields[cname, f] else []
            bad += [type_mismatch(ctype, t._type_ if is_arr else t, mirrors) if is_arr == arr else "an array on one side only"]
            out += [(f"{cname}.{f}", b) for b in bad if b]
    return out


def check_slots(cname, slots, n_slots, abi):
    """a struct of 8-byte fields that the binding addresses by slot index, slots {field: index or None}"""
    out = [(cname, f"{n_slots} slots, header sizeof {abi.sizes[cname]}")] if 8 * n_slots != abi.sizes[cname] else []
    return out + [(f"{cname}.{f}", f"slot {i}, header (offset, size) {abi.fields[cname, f]}")
                  for f, i in slots.items() if i is None or abi.fields[cname, f] != (8 * i, 8)]


def check_structs(mirrors, abi, slot_structs=()):
    """every mirror names its struct; every struct of the header has exactly one mirror (or is one of `slot_structs`); all agree"""
    out = [(t.__name__, "the docstring does not start with the C type's name, or the header has no such struct")
           for t, c in mirrors.items() if c not in abi.structs]
    for cname in abi.structs:
        mine = [t for t, c in mirrors.items() if c == cname]
        out += [(cname, f"{len(mine)} mirrors")] if len(mine) != (0 if cname in slot_structs else 1) else []
        out += [f for t in mine for f in check_struct(cname, t, abi, mirrors)]
    return out


def check_signatures(signatures, abi, mirrors):
    """{name: (restype, argtypes)} against the header's prototypes: the names, the arity, each parameter's and the return's class"""
    out = [(n, "in the header or the table only") for n in set(abi.prototypes) ^ set(signatures)]
    for name, (ret, params) in abi.prototypes.items():
        res, args = signatures.get(name, (None, None))
        if args is not None and len(args) != len(params):
            out.append((name, f"{len(args)} arguments, header {len(params)}"))
        elif args is not None:
            bad = [(f"{name} return", type_mismatch(ret, res, mirrors))]
            bad += [(f"{name}.{p}", type_mismatch(ctype, a, mirrors)) for (ctype, p), a in zip(params, args)]
            out += [b for b in bad if b[1]]
    return out


def check_constants(namespace, abi, unmirrored):
    """every header constant DAL3_X equals the int namespace["X"], or stands in `unmirrored` because there is none"""
    out = [(k, "listed as unmirrored, not in the header") for k in unmirrored if k not in abi.constants]
    for k, v in abi.constants.items():
        mine = namespace.get(k[len("DAL3_"):])
        if isinstance(mine, int) and not isinstance(mine, bool):
            out += [(k, f"{mine}, header {v}")] if mine != v else []
            out += [(k, "mirrored, yet listed as unmirrored")] if k in unmirrored else []
        elif k not in unmirrored:
            out.append((k, "neither mirrored nor listed as unmirrored"))
    return out
