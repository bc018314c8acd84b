#!/usr/bin/env python3
"""Which gfx950 device functions of two built libraries differ (no GPU needed): the comparison a refactor of shared
device code is judged by (MEASUREMENTS.md sections O3, H1, O6).

    python tools/isa_diff.py parent/libstb_amd.so libstb_amd/lib/libstb_amd.so

Every code object of each library (tools/kernel_regs.py's code_objects) is disassembled with llvm-objdump; addresses,
encodings, comments and the <symbol+offset> notes behind branch targets are dropped, and what is left of a function is
compared line by line.  Prints how many functions are equal, then the demangled name and both line counts of every
one that differs or exists on one side only.  It compares and does nothing else."""
import re
import subprocess
import sys
import tempfile

from kernel_regs import LLVM, code_objects, demangle


def functions(lib):
    """{demangled name: [instruction lines]} over all code objects of lib (a name met again gets ' #2', ' #3', ..)"""
    found, order = {}, []
    for img in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", f.name],
                                 capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:\s*$", line)
            if m:
                name, n = m.group(1), 1
                while (name if n == 1 else f"{name} #{n}") in found:
                    n += 1
                cur = name if n == 1 else f"{name} #{n}"
                found[cur] = []
                order.append(cur)
                continue
            if cur is None:
                continue
            line = re.sub(r"//.*$", "", line)           # encodings and addresses travel as comments
            line = re.sub(r"\s*<[^>]*>\s*$", "", line)  # the note behind a branch target
            line = " ".join(line.split())
            if line:
                found[cur].append(line)
    heads = [re.sub(r" #\d+$", "", n) for n in order]
    tails = [n[len(h):] for n, h in zip(order, heads)]
    return {re.sub(r"^void ", "", d) + t: found[n] for d, t, n in zip(demangle(heads), tails, order)}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    equal = sum(1 for n in a if n in b and a[n] == b[n])
    print(f"# {len(a)} device functions in {sys.argv[1]}, {len(b)} in {sys.argv[2]}: {equal} equal")
    for n in sorted(set(a) | set(b)):
        if n in a and n in b and a[n] == b[n]:
            continue
        la = len(a[n]) if n in a else "-"
        lb = len(b[n]) if n in b else "-"
        print(f"{la:>7} {lb:>7}  {n[:160]}")


if __name__ == "__main__":
    main()
