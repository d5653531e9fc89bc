"""The one check that a header of include/ and its ctypes binding agree (no GPU: the library is only loaded)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def header_text(header):
    """The header without its comments."""
    text = open(os.path.join(INCLUDE, header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def prototypes(header, prefix):
    """{name: (return type, number of parameters)} of the functions of the header whose names match `prefix`."""
    found = re.findall(r"(?m)^[ \t]*((?:const[ \t]+)?\w+[ \t]*\**)[ \t]*\b(%s)[ \t]*\(([^)]*)\)[ \t]*;" % prefix, header_text(header))
    return {name: (re.sub(r"\s+", "", ret.replace("const", "")), 0 if params.strip() == "void" else params.count(",") + 1)
            for ret, name, params in found}


def layout(header, structs, constants):
    """The lines a C program prints: per struct its name, sizeof and every offsetof, then the constants; compiled as C++17
    and as C99 with -Wall -Werror, and both must print the same."""
    lines = []
    for cname, st in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        lines += ['printf(" %s:%%zu", offsetof(%s, %s));' % (f, cname, f) for f, *_ in st._fields_]
        lines.append('printf("\\n");')
    lines += ['printf("%s %%lld\\n", (long long)(%s));' % (c, c) for c in constants]
    body = '#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) { %s return 0; }\n' % (os.path.join(INCLUDE, header), " ".join(lines))
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for src, cmd in (("layout.cpp", ["g++", "-std=c++17"]), ("layout.c", ["gcc", "-std=c99", "-Wall", "-Werror"])):
            path = os.path.join(tmp, src)
            with open(path, "w") as f:
                f.write(body)
            subprocess.check_call(cmd + ["-o", path + ".exe", path])
            outs.append(subprocess.run([path + ".exe"], capture_output=True, text=True, check=True).stdout.splitlines())
    assert outs[0] == outs[1]
    return outs[0]


def check_functions(header, module, prefix):
    """The prototypes of include/<header> whose names match the regex `prefix`, comments stripped, are module.EXPORTS; each
    resolves in the built library, has an entry in module.PROTOTYPES and, bound by module.lib(), as many argtypes as the
    prototype has parameters ((void) is none) and the restype of its return type: None for void, c_char_p for const char*,
    c_void_p for another pointer, c_int for int.  (No header returns another integer type; one that did would be named here
    and in its table.)  Returns the number of prototypes."""
    from defuse_amd import dsa
    protos = prototypes(header, prefix)
    declared = set(re.findall(r"\b(%s)\s*\(" % prefix, header_text(header)))
    assert declared == set(protos), "a declaration of %s the prototype parser does not read" % header
    assert declared == set(module.EXPORTS) and len(module.EXPORTS) == len(declared)
    plain = ctypes.CDLL(dsa.LIB_PATH)
    bound = module.lib()
    restype = {"void": None, "char*": ctypes.c_char_p, "int": ctypes.c_int}
    for name, (ret, n_params) in sorted(protos.items()):
        assert getattr(plain, name) is not None, name
        assert name in module.PROTOTYPES, "%s is not in the PROTOTYPES table of %s" % (name, module.__name__)
        fn = getattr(bound, name)
        assert len(fn.argtypes) == n_params, "%s: %d argtypes for %d parameters" % (name, len(fn.argtypes), n_params)
        want = ctypes.c_void_p if ret.endswith("*") and ret != "char*" else restype[ret]
        assert fn.restype is want, "%s: restype %r for a function returning %s" % (name, fn.restype, ret)
    return len(protos)


def check(header, module, prefix, constants=None, dtypes=()):
    """include/<header> against its binding `module`: check_functions, and
      - sizeof and every offsetof of module.STRUCTS (C name -> ctypes struct), as g++ and gcc -std=c99 see them, equal the
        ctypes structs';
      - every (struct, dtype) of `dtypes` has the same field names, offsets and size;
      - `constants` (C name -> Python value) are equal.
    Returns ([sizeof of every struct, in the order of module.STRUCTS], the number of prototypes)."""
    structs, constants = module.STRUCTS, constants or {}
    got = layout(header, structs, constants)
    assert len(got) == len(structs) + len(constants)
    for line, (cname, st) in zip(got, structs.items()):
        assert line == "%s %d" % (cname, ctypes.sizeof(st)) + "".join(" %s:%d" % (f, getattr(st, f).offset) for f, *_ in st._fields_)
    assert got[len(structs):] == ["%s %d" % (c, v) for c, v in constants.items()]
    for st, dt in dtypes:
        assert ctypes.sizeof(st) == dt.itemsize, st
        assert [(f, getattr(st, f).offset) for f, *_ in st._fields_] == [(f, dt.fields[f][1]) for f in dt.names], st
    return [ctypes.sizeof(st) for st in structs.values()], check_functions(header, module, prefix)
