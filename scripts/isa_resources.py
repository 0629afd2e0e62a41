#!/usr/bin/env python3
"""scripts/isa_resources.py [OUT [ASM_DIR [FILES]]] -- compile the kernel files for gfx950 with --save-temps and list
what the code object's metadata says every kernel uses (VGPRs, AGPRs, SGPRs, static LDS, scratch,
spills) plus the occupancy that follows (512 VGPRs per SIMD lane on CDNA4, granule 8, at most 8
waves per SIMD).  Runs without a GPU.  The summary is written to OUT (default
profiles/isa_resources.txt) so that statements about registers / occupancy in DESIGN.md can be
checked against the compiler's own numbers rather than against profiler dispatch fields
(rocprofv3's VGPR_Count column reports the arch-VGPR allocation only and LDS_Block_Size does
not include dynamic LDS).  With ASM_DIR the assembly is kept there, a directory per file, for
scripts/isa_instr_diff.py.  FILES (comma-separated, e.g. similarity_kernels) restricts the run to those kernel
files (ASM_DIR may be "" then)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_FILES = ("hash_kernels", "kernels", "scan_findere", "topk_kernels", "build_kernels", "group_kernels", "fill_kernels",
                "prevalence_kernels", "weighted_kernels", "set_kernels", "set_count_kernels", "coverage_kernels", "window_kernels", "presence_kernels",
                "fetch_kernels", "best_kernels", "similarity_kernels")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "isa_resources.txt")
    keep = (sys.argv[2] if len(sys.argv) > 2 else None) or None
    files = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else KERNEL_FILES
    # K1 (hash_kernels.hip), the scan kernels (kernels.hip: the kernel and its plain instantiations,
    # scan_findere.hip the findere ones), K3 (topk_kernels.hip), construction (build_kernels.hip), the grouped-search
    # kernels (group_kernels.hip: accumulate, select, zero) and the filter-fill
    # kernels (fill_kernels.hip: count, its load-only probe, zero), the prevalence kernels (prevalence_kernels.hip), the
    # kernels of the weighted search (weighted_kernels.hip: weights, weighted scan), the document-set kernels
    # (set_kernels.hip: set presence, select; set_count_kernels.hip: set count, quorum select), the coverage scan (coverage_kernels.hip), the window scan
    # (window_kernels.hip), and the other readers of K1's
    # row-index table (row_table.hpp): the presence kernel and the out-of-core fetch kernels; the best-of-group kernels
    # (best_kernels.hip: best member, merge of partial states, select, init); the document-similarity kernels
    # (similarity_kernels.hip: reference bits per row, the shared-bits sweep in its two variants, zero)
    asm = ""
    for name in files:
        src = os.path.join(ROOT, "cobs_amd", "csrc", name + ".hip")
        with tempfile.TemporaryDirectory() as tmp:
            if keep:
                tmp = os.path.join(os.path.abspath(keep), name)
                os.makedirs(tmp, exist_ok=True)
            subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                                   "-I" + os.path.dirname(src), "--save-temps", "-c", src, "-o", "k.o"], cwd=tmp,
                                  stderr=subprocess.DEVNULL)
            asm += open(os.path.join(tmp, name + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read() + "\n"
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    rows = []
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", asm, re.S):
        blk = m.group(0)

        def g(k):
            r = re.search(r"\.%s:\s*(\S+)" % k, blk)
            return r.group(1) if r else "?"
        sym = g("name")
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        dem = dem.replace("cobs_amd::", "").replace("(anonymous namespace)::", "").replace("unsigned char", "u8").replace("unsigned short", "u16") \
                 .replace("unsigned int", "u32").replace("unsigned long", "u64")
        dem = re.sub(r"\(.*\)$", "", dem).replace("void ", "")
        vg, ag = int(g("vgpr_count")), int(g("agpr_count"))
        # unified register file: arch VGPRs + AGPRs, allocated in granules of 8, 512 per SIMD lane
        alloc = (vg + 7) // 8 * 8      # .vgpr_count already includes the AGPRs (unified file)
        waves = min(8, 512 // max(alloc, 1))
        rows.append((dem, vg, ag, int(g("sgpr_count")), int(g("group_segment_fixed_size")),
                     int(g("private_segment_fixed_size")), g("vgpr_spill_count"), waves))
    rows.sort()
    lines = ["# %s @ %s, hipcc -O3 --offload-arch=gfx950; from the code object metadata (.s of --save-temps)"
             % (", ".join(n + ".hip" for n in files), head),
             "# static_lds excludes the dynamic LDS a launch adds (scan_kernel: merge buffers + expansion table)",
             "%-64s %5s %5s %5s %10s %8s %6s %10s" % ("kernel", "vgpr", "agpr", "sgpr", "static_lds", "scratch", "spill",
                                                     "waves/SIMD")]
    for r in rows:
        lines.append("%-64s %5d %5d %5d %10d %8d %6s %10d" % r)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
