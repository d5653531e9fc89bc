"""The vector-memory instructions and the waits on them in one kernel of an assembly file, in program order.

    python profiles/microbench/vmem_waits.py a.s 'k_fill_fast<0, false, 56>' [--lgkm]

One line per global / flat / scratch access, per s_waitcnt that names vmcnt (with --lgkm: every s_waitcnt), per label,
branch and barrier; between them the number of other instructions, so that a loop reads as: where its loads are issued,
how much is issued behind them, and where they are waited for.  Line numbers are those of the kernel's normalised
instruction stream (isa_diff.py).
"""
import re
import sys

import isa_diff


def main(argv):
    ks = isa_diff.kernels(argv[1])
    dem = isa_diff.demangle(sorted(ks))
    lgkm = "--lgkm" in argv
    for n in sorted(ks):
        if isa_diff.base(dem[n]).endswith(argv[2]):
            body, stats = ks[n]
            print("== %s: %d instructions, %s" % (isa_diff.base(dem[n]), len(body), stats))
            other = 0
            for i, ln in enumerate(body):
                op = ln.split()[0]
                keep = (re.match(r"(global|flat|scratch|buffer)_", op) or ln.endswith(":") or op.startswith("s_cbranch") or op in ("s_branch", "s_barrier", "s_endpgm")
                        or (op == "s_waitcnt" and (lgkm or "vmcnt" in ln)))
                if keep:
                    if other:
                        print("        ... %d" % other)
                    other = 0
                    print("%6d  %s" % (i, ln))
                else:
                    other += 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
