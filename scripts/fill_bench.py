#!/usr/bin/env python3
"""scripts/fill_bench.py -- what the filter-fill sweep (cobs_gpu_doc_bits) costs, beside its load-only probe.

Two resident procedural indexes: C3 (8 sub-indexes of 1568-byte pages, 18.4 GB) and the configs[3] geometry (245
sub-indexes of 512-byte pages).  In one process, alternating, several repetitions each: the counting kernel (the
library's own events, cobs_gpu_doc_bits_ms; before every repetition one short text is planted into document 0, which
drops the handle's cached counts so that the sweep runs again) and the probe (scripts/probes/fill_probe.py: the same loads, one XOR per load, one store per lane).  The yardstick is the
probe on the same box in the same process.  Optionally (--budget-gib) the wall time of doc_bits on a budgeted handle
beside one whole-chunk search pass over the same file: both are bound by the same PCIe copies.
One JSON document on stdout, the same in --out (default profiles/fill_bench.json).

    python scripts/fill_bench.py [--reps 5] [--scale 1.0] [--c4-scale 0.25] [--budget-gib 6] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from scripts.probes.fill_probe import probe_ms  # noqa: E402


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def measure(name, cfg, reps):
    s = bench.make_index(cfg, 0)
    text = bench.make_queries(1, 40, seed=7)[0]
    kernel, probe, nbytes = [], [], 0
    for rep in range(reps + 1):
        s.plant(text, [0], 1000, salt=rep)            # changes (at most) a few bits of document 0: the cache is dropped
        before = s.doc_bits_ms()
        s.doc_bits()
        after = s.doc_bits_ms()
        assert after["passes"] == before["passes"] + 1
        p = probe_ms(s)
        if rep == 0:
            continue                                   # warm-up
        kernel.append(after["kernel_ms"] - before["kernel_ms"])
        nbytes = after["bytes_read"] - before["bytes_read"]
        probe.append(p)
    out = {"index": name, "bytes_read": nbytes, "kernel_ms": stats(kernel), "probe_ms": stats(probe),
           "kernel_gb_s": nbytes / statistics.median(kernel) / 1e6, "probe_gb_s": nbytes / statistics.median(probe) / 1e6,
           "kernel_over_probe": statistics.median(kernel) / statistics.median(probe)}
    s.close()
    return out


def budgeted(cfg, budget, queries):
    s = bench.make_index(cfg, 0, hbm_budget=budget)
    s.set_tuning("row_fetch", 0)                       # the search pass copies every streamed chunk whole
    t0 = time.perf_counter()
    s.doc_bits()
    t_bits = time.perf_counter() - t0
    ms = s.doc_bits_ms()
    s.search_hits(queries[:1], 0.9, 1)                 # warm the pass's workspaces
    t0 = time.perf_counter()
    s.search_hits(queries, 0.9, 1)
    t_pass = time.perf_counter() - t0
    out = {"hbm_budget": budget, "stream_plan": list(s.stream_plan()), "doc_bits_wall_ms": t_bits * 1e3,
           "doc_bits_kernel_ms": ms["kernel_ms"], "doc_bits_pcie_ms": ms["pcie_ms"], "doc_bits_bytes_read": ms["bytes_read"],
           "search_pass_wall_ms": t_pass * 1e3}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--c4-scale", type=float, default=0.25)
    ap.add_argument("--budget-gib", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_bench.json"))
    args = ap.parse_args()
    res = {"reps": args.reps, "runs": []}
    res["runs"].append(measure("C3 procedural, scale %g" % args.scale, bench.c3_config(args.scale), args.reps))
    res["runs"].append(measure("configs[3] geometry (245 sub-indexes, 512-byte pages), scale %g" % args.c4_scale,
                               bench.c4_config(args.c4_scale), args.reps))
    if args.budget_gib > 0:
        res["budgeted"] = budgeted(bench.c3_config(args.scale), int(args.budget_gib * (1 << 30)), bench.make_queries(64, 1000))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
