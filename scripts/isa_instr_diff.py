#!/usr/bin/env python3
"""scripts/isa_instr_diff.py BEFORE_DIR AFTER_DIR [OUT] -- instructions per kernel in two sets of gfx950 assembly files
(the *-hip-amdgcn-amd-amdhsa-gfx950.s that `hipcc --save-temps -c FILE.hip` leaves; every .s below each directory is
read, whatever translation unit it came from).  Checks a refactor that moves kernels between files: the kernel name
sets must be equal, and the table says how far each kernel's instruction count moved.  Runs without a GPU."""
import os
import re
import subprocess
import sys


def kernels_of(root):
    """{mangled kernel name: instruction count} over every .s under root"""
    out = {}
    for d, _, files in os.walk(root):
        for fn in files:
            if not fn.endswith(".s"):
                continue
            text = open(os.path.join(d, fn)).read()
            names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
            for name in names:
                m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
                body = m.group(1) if m else ""
                # an instruction line: a tab, then a mnemonic (labels, directives and comments start otherwise)
                out[name] = sum(1 for ln in body.split("\n") if re.match(r"\s+[a-z]", ln) and not ln.lstrip().startswith("."))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = []
    for d in r[:len(names)]:
        d = d.replace("cobs_amd::", "").replace("(anonymous namespace)::", "").replace("unsigned char", "u8") \
             .replace("unsigned short", "u16").replace("unsigned int", "u32").replace("unsigned long", "u64")
        short.append(re.sub(r"\(.*\)$", "", d).replace("void ", ""))
    return dict(zip(names, short))


def main():
    before, after = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    only_b, only_a = sorted(set(before) - set(after)), sorted(set(after) - set(before))
    names = sorted(set(before) & set(after))
    dem = demangle(sorted(set(before) | set(after)))
    lines = ["# instructions per kernel (from its label to .Lfunc_end), hipcc -O3 --offload-arch=gfx950, before -> after",
             "# kernels: %d before, %d after, %d in both; only before: %d, only after: %d"
             % (len(before), len(after), len(names), len(only_b), len(only_a))]
    lines += ["# ONLY BEFORE: " + dem[n] for n in only_b] + ["# ONLY AFTER: " + dem[n] for n in only_a]
    moved = [n for n in names if before[n] != after[n]]
    lines.append("# kernels whose count moved: %d (largest |delta|: %d)"
                 % (len(moved), max([abs(after[n] - before[n]) for n in moved] or [0])))
    lines.append("%-64s %8s %8s %6s" % ("kernel", "before", "after", "delta"))
    for n in sorted(names, key=lambda n: dem[n]):
        lines.append("%-64s %8d %8d %+6d" % (dem[n], before[n], after[n], after[n] - before[n]))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(text)
    sys.stdout.write(text if len(sys.argv) <= 3 else "\n".join(lines[:3 + len(only_b) + len(only_a)]) + "\n")
    return 1 if only_b or only_a else 0


if __name__ == "__main__":
    sys.exit(main())
