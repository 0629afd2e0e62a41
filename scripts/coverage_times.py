#!/usr/bin/env python3
"""scripts/coverage_times.py -- what the coverage scan (cobs_gpu_search_coverage) costs beside K2 on the same batch.

The C3 procedural geometry with planted documents and the headline batch (10 000 x 1000-position queries cut from the
planted sequences) at threshold 0.8.  In one process, on one handle, alternating, several repetitions each (every
measured call follows an unmeasured call of its own kind): the stages of the coverage call (cobs_gpu_coverage_ms: K1,
coverage scan) and the plain scan of search_arrays at the same threshold (the handle's "scan" timer: K2 with its
threshold epilogue) -- the yardstick, code the coverage call does not change.  Algorithmic bytes of the coverage scan:
K2's row bytes (positions x H x (z + 1) x row bytes per sub-index).

Both calls run at findere z (--findere, default 3), not at z = 0: the procedural filters are 30 % full, so at z = 0 a
random document holds a position with probability 0.3 and a base stays uncovered with probability 0.7^31 -- every one
of the 100 000 documents covers practically every base of every query, and a thresholded coverage call would return
10^9 records.  At z = 3 a random position is set with probability 0.3^4 and only the planted documents reach 0.8.
A text table on stdout, the same in --out (default profiles/coverage_times.txt).

With --kernel-stats FILE the script also starts ONE run of itself (--reps 1, a fresh child process) under
`rocprofv3 --kernel-trace --stats` (no counters in that run) and writes the kernel table's rows of the two calls to FILE
(default profiles/coverage_kernel_stats.txt).

    python scripts/coverage_times.py [--reps 5] [--queries 10000] [--kmers 1000] [--scale 1.0] [--threshold 0.8] [--findere 3]
                                     [--out FILE] [--kernel-stats [FILE]]
"""
import argparse
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

STATS_DEFAULT = os.path.join(ROOT, "profiles", "coverage_kernel_stats.txt")


def kernel_stats(args):
    """one run of this script under rocprofv3 in a child process; the kernel table to args.kernel_stats"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "cov", "--",
               sys.executable, os.path.abspath(__file__), "--reps", "1", "--queries", str(args.queries), "--kmers", str(args.kmers),
               "--scale", str(args.scale), "--threshold", str(args.threshold), "--findere", str(args.findere), "--out", os.path.join(tmp, "times.txt")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        rows = open(found[0]).read().splitlines()
    keep = [rows[0]] + [r for r in rows[1:] if "coverage_scan_kernel" in r or "scan_kernel<" in r or "hash_kernel" in r]
    head = ["# rocprofv3 --kernel-trace --stats -- python scripts/coverage_times.py --reps 1: the kernel table, the rows of the coverage call and its",
            "# yardstick (C3 procedural scale %g, %d x %d-k-mer planted queries, threshold %g, findere %d; durations per launch; search_arrays runs K2 in several launches per call)"
            % (args.scale, args.queries, args.kmers, args.threshold, args.findere)]
    with open(args.kernel_stats, "w") as f:
        f.write("\n".join(head + keep) + "\n")
    sys.stdout.write("\n".join(keep) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--findere", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage_times.txt"))
    ap.add_argument("--kernel-stats", nargs="?", const=STATS_DEFAULT, default=None)
    args = ap.parse_args()
    cfg = bench.c3_config(args.scale)
    plants = bench.planted_documents(cfg, args.kmers)
    cfg["plants"] = plants
    queries = bench.planted_queries(plants, args.queries, args.kmers)
    s = bench.make_index(cfg, 0)
    s.set_findere(args.findere)
    cov, hash_ms, k2 = [], [], []
    hits_c = hits_k2 = 0
    for rep in range(args.reps):
        # every measured call follows an unmeasured call of its own kind: clocks and caches as in a stream of such calls
        s.search_coverage_arrays(queries, args.threshold, 0)
        s.coverage_ms()
        offs, hits = s.search_coverage_arrays(queries, args.threshold, 0)
        t = s.coverage_ms()
        assert t["passes"] == 1, t               # (one run of one pass: the result buffer of the mirror was large enough)
        hits_c = int(offs[-1])
        s.search_arrays(queries, args.threshold, 0)
        s.timers(reset=True)
        offs, hits = s.search_arrays(queries, args.threshold, 0)
        hits_k2 = int(offs[-1])
        k2.append(s.timers(reset=True)["scan"] * 1e3)
        cov.append(t["scan_ms"])
        hash_ms.append(t["hash_ms"])
        print("rep %d: coverage scan %.3f ms (%d hits), search_arrays scan %.3f ms (%d hits)" % (rep, cov[-1], hits_c, k2[-1], hits_k2), flush=True)
    med = statistics.median
    positions = len(queries) * args.kmers
    row_bytes = cfg["page_size"] * len(cfg["signature_sizes"]) * cfg["num_hashes"]
    scan_bytes = positions * row_bytes * (args.findere + 1)
    lines = ["# scripts/coverage_times.py: C3 procedural (scale %g), %d queries x %d k-mers from planted sequences, threshold %g, "
             "findere %d, %d repetitions (median [min .. max], ms)" % (args.scale, len(queries), args.kmers, args.threshold, args.findere, args.reps),
             "# both calls at findere %d: the yardstick is search_arrays' scan at that z (the findere scan for z > 0), NOT the z = 0 headline K2"
             % args.findere,
             "coverage hash_ms        %9.3f  [%9.3f .. %9.3f]" % (med(hash_ms), min(hash_ms), max(hash_ms)),
             "coverage scan_ms        %9.3f  [%9.3f .. %9.3f]" % (med(cov), min(cov), max(cov)),
             "scan of search_arrays   %9.3f  [%9.3f .. %9.3f]" % (med(k2), min(k2), max(k2)),
             "hits: coverage %d, plain %d" % (hits_c, hits_k2),
             "coverage scan: %.3e algorithmic bytes, %.3f TB/s; ratio to the search_arrays scan's time at the same findere %.3f" %
             (scan_bytes, scan_bytes / med(cov) / 1e9, med(cov) / med(k2))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    s.close()
    if args.kernel_stats:
        kernel_stats(args)


if __name__ == "__main__":
    main()
