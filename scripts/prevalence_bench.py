#!/usr/bin/env python3
"""scripts/prevalence_bench.py -- what the prevalence kernel (cobs_gpu_prevalence) costs, beside the scan of the same batch.

The C3 procedural geometry with the headline batch (10 000 x 1000-k-mer queries, one hash function) and the three-hash
shape.  In one process, alternating, several repetitions each: the prevalence kernel at findere z = 0 and z = 3 (the
library's own events, cobs_gpu_prevalence_ms) and the existing K2 scan of the same batch on the same handle
(Batch.run(0.0), cobs_gpu_batch_kernel_ms) -- the yardstick, code the prevalence call does not touch.
Algorithmic bytes of the prevalence kernel: positions x H x row bytes per held sub-index (K2's reads for the batch); its
writes are 4 bytes per position.  One JSON document on stdout, the same in --out (default profiles/prevalence_bench.json).

    python scripts/prevalence_bench.py [--reps 5] [--queries 10000] [--kmers 1000] [--scale 1.0] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import cobs_amd  # noqa: E402


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def measure(name, cfg, queries, kmers, reps):
    s = bench.make_index(cfg, 0)
    b = cobs_amd.Batch(s)
    b.set_queries(queries)
    row_bytes = cfg["page_size"] if cfg["kind"] == "compact" else (cfg["num_docs"] + 7) // 8
    pages = len(cfg["signature_sizes"])
    prev = {0: [], 3: []}
    hash_ms = {0: [], 3: []}
    scan = []
    for rep in range(reps + 1):
        for z in (0, 3):
            s.set_findere(z)
            s.prevalence_ms()
            s.prevalence_arrays(queries)
            t = s.prevalence_ms()
            if rep:
                prev[z].append(t["kernel_ms"])
                hash_ms[z].append(t["hash_ms"])
        s.set_findere(0)
        b.kernel_ms()
        b.run(0.0)
        b.sync()
        ms = b.kernel_ms()
        if rep:
            scan.append(ms["scan_ms"])
    out = {"index": name, "queries": len(queries), "kmers": kmers, "num_hashes": cfg["num_hashes"], "k2_scan_ms": stats(scan)}
    k2 = statistics.median(scan)
    for z in (0, 3):
        positions = len(queries) * (kmers - z)
        nbytes = positions * cfg["num_hashes"] * row_bytes * pages
        ms = statistics.median(prev[z])
        out["z%d" % z] = {"kernel_ms": stats(prev[z]), "hash_ms": stats(hash_ms[z]), "algorithmic_bytes": nbytes,
                          "bytes_written": 4 * positions, "algorithmic_tb_s": nbytes / ms / 1e9,
                          "fraction_of_8_tb_s": nbytes / ms / 1e9 / 8.0, "ratio_to_k2": ms / k2}
    b.close()
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prevalence_bench.json"))
    args = ap.parse_args()
    queries = bench.make_queries(args.queries, args.kmers)
    res = {"reps": args.reps, "runs": []}
    for h in (1, 3):
        cfg = bench.c3_config(args.scale)
        cfg["num_hashes"] = h
        res["runs"].append(measure("C3 procedural, scale %g, H = %d" % (args.scale, h), cfg, queries, args.kmers, args.reps))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
