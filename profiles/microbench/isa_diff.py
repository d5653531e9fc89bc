"""Compare the device code of two builds of dsa_api.hip, kernel by kernel.

    hipcc <LIB_FLAGS without -shared> <effective_dsa_flags()> --cuda-device-only -S -o a.s defuse_amd/csrc/dsa_api.hip
    python profiles/microbench/isa_diff.py a.s b.s [--show NAME ...]

A kernel is "same" if its instruction stream is equal once local label numbers are renumbered in order of appearance.
Kernels are matched by mangled name; those whose signature changed (no such name on the other side) are matched by their
demangled name without the parameter list, and their registers, scratch, occupancy and code size are printed for both
builds.  --show NAME prints a unified diff of the instruction streams of every kernel whose demangled name contains NAME.
"""
import difflib
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (instructions, {NumVgprs, ScratchSize, Occupancy, codeLenInByte})} of the .amdhsa kernels in an assembly file"""
    out, name, body = {}, None, []
    lines = open(path, errors="replace").read().split("\n")
    is_kernel = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if name is None and m and m.group(1) in is_kernel:
            name, body = m.group(1), []
        elif name is not None:
            if ln.startswith(".Lfunc_end"):
                stats = {}
                for k in range(i, min(i + 60, len(lines))):
                    s = re.match(r"^; (NumVgprs|ScratchSize|Occupancy|codeLenInByte)(?::| =) (\d+)", lines[k])
                    if s:
                        stats[s.group(1)] = int(s.group(2))
                out[name] = (normalise(body), stats)
                name = None
            else:
                body.append(ln)
        i += 1
    return out


def normalise(body):
    labels, res = {}, []
    for ln in body:
        ln = ln.split(";")[0].rstrip()
        if not ln.strip() or re.match(r"^\s*\.(p2align|loc|file|cfi\w*)\b", ln):
            continue
        ln = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln)
        res.append(ln.strip())
    return res


def demangle(names):
    txt = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.split("\n")
    return dict(zip(names, txt))


def base(dem):
    """demangled name without its parameter list: 'void dsa::k_emit_listed<true>'"""
    depth = 0
    for k, ch in enumerate(dem):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return dem[:k]
    return dem


def main(argv):
    a, b = kernels(argv[1]), kernels(argv[2])
    show = argv[argv.index("--show") + 1:] if "--show" in argv else []
    dem = demangle(sorted(set(a) | set(b)))
    same = [n for n in a if n in b and a[n][0] == b[n][0]]
    diff = [n for n in a if n in b and a[n][0] != b[n][0]]
    print("%d kernels in %s, %d in %s; %d with the same name and the same instruction stream" % (len(a), argv[1], len(b), argv[2], len(same)))
    for n in diff:
        print("DIFFERENT  %s" % dem[n])
    only_a = {base(dem[n]): n for n in a if n not in b}
    only_b = {base(dem[n]): n for n in b if n not in a}
    for key in sorted(set(only_a) | set(only_b)):
        na, nb = only_a.get(key), only_b.get(key)
        if not (na and nb):
            print("UNMATCHED  %s (only in %s)" % (key, argv[1] if na else argv[2]))
            continue
        sa, sb = a[na][1], b[nb][1]
        print("re-signed  %s: %s" % (key, "same instruction stream" if a[na][0] == b[nb][0] else "%d -> %d instructions" % (len(a[na][0]), len(b[nb][0]))))
        for f in ("NumVgprs", "ScratchSize", "Occupancy", "codeLenInByte"):
            print("             %-14s %6s -> %6s" % (f, sa.get(f), sb.get(f)))
    for want in show:
        for n in list(diff) + [only_a[k] for k in only_a if k in only_b]:
            if want in dem[n]:
                m = n if n in b else only_b[base(dem[n])]
                print("\n".join(difflib.unified_diff(a[n][0], b[m][0], "a: " + dem[n], "b: " + dem[m], lineterm="", n=4)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
