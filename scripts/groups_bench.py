#!/usr/bin/env python3
"""scripts/groups_bench.py -- what grouped search costs beside the two ways a caller had to get the same totals.

The procedural C3 index with planted documents and the batch of `bench.py --full`'s end_to_end (10 000 queries of 1000
k-mers with hits).  In one process, alternating, several repetitions each:
  groups_one     cobs_gpu_search_groups, the whole batch as ONE group (the split-span / atomic path)
  groups_pairs   cobs_gpu_search_groups, groups of two (the one-writer path)
  search_batch   cobs_gpu_search_batch at the same threshold (per-query hits only: what existed before)
  rows_to_host   every score row to the host and a numpy sum over the group (the only way to a group's totals before)
with the library's own timers of the accumulate and select kernels (Search.groups_ms), the K2 scan time of the same batch
(Batch.kernel_ms) and the accumulate kernel's bytes read per second.  The condition the design sets: the accumulate
kernel takes less time than the K2 scan of the same pass.  The totals of groups_one are checked against the numpy sum.
One JSON line on stdout, the same in --out (default profiles/groups_bench.json).

    python scripts/groups_bench.py [--queries 10000] [--kmers 1000] [--reps 5] [--scale 1.0] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402
from cobs_amd import Batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups_bench.json"))
    args = ap.parse_args()

    cfg = bench.c3_config(args.scale)
    cfg["plants"] = bench.planted_documents(cfg, args.kmers)
    s = bench.make_index(cfg, 0)
    queries = bench.planted_queries(cfg["plants"], args.queries, args.kmers)
    nq = len(queries)
    one = np.array([0, nq], dtype=np.uint64)
    pairs = np.minimum(np.arange(0, nq + 2, 2), nq).astype(np.uint64)
    pairs = pairs[:int(np.argmax(pairs == nq)) + 1]
    b = Batch(s)
    b.set_queries(queries)

    t = {"groups_one": [], "groups_pairs": [], "search_batch": [], "rows_to_host": []}
    k = {"one_acc": [], "one_sel": [], "one_order": [], "pairs_acc": [], "pairs_sel": [], "pairs_order": [], "scan": []}
    res_one = rows_sum = None
    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        t0 = time.perf_counter()
        res_one = s.search_groups_arrays(queries, one, args.threshold, args.threshold, 0)
        t1 = time.perf_counter()
        m1 = s.groups_ms()
        t2 = time.perf_counter()
        s.search_groups_arrays(queries, pairs, args.threshold, args.threshold, 0)
        t3 = time.perf_counter()
        m2 = s.groups_ms()
        t4 = time.perf_counter()
        s.search_arrays(queries, args.threshold, 0)
        t5 = time.perf_counter()
        b.run(0.0)
        b.sync()
        rows = b.counts_tensor().cpu().numpy()
        rows_sum = rows.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[rows.dtype.itemsize]).sum(axis=0, dtype=np.uint64)
        t6 = time.perf_counter()
        scan = b.kernel_ms()["scan_ms"]
        if keep:
            t["groups_one"].append(t1 - t0)
            t["groups_pairs"].append(t3 - t2)
            t["search_batch"].append(t5 - t4)
            t["rows_to_host"].append(t6 - t5)
            for name, m in (("one", m1), ("pairs", m2)):
                k[name + "_acc"].append(m["accumulate_ms"])
                k[name + "_sel"].append(m["select_ms"])
                k[name + "_order"].append(m["order_ms"])
            k["scan"].append(scan)
    # self-check: the one group's sums are the column sums of the score rows (the documents of the one file are slots 0 ..)
    offs, hits, pos = res_one
    _o, best, _p = s.search_groups_arrays(queries, one, 0.0, 0.0, 1000)
    ok = len(best) == 1000 and all(int(rows_sum[int(d)]) == int(sc) and int(v) == nq for (_f, d, sc, v) in best.tolist())

    def spread(v, scale=1.0):
        return {"median": round(statistics.median(v) * scale, 4), "min": round(min(v) * scale, 4), "max": round(max(v) * scale, 4)}

    _p, elem_bytes, _stride = b.counts_device()
    matrix_bytes = nq * s.local_counts * elem_bytes
    acc_one, acc_pairs, scan = statistics.median(k["one_acc"]), statistics.median(k["pairs_acc"]), statistics.median(k["scan"])
    out = {
        "name": "groups_bench", "queries": nq, "kmers": args.kmers, "threshold": args.threshold, "scale": args.scale,
        "documents": int(s.total_counts), "score_bytes": int(elem_bytes), "score_matrix_bytes": int(matrix_bytes),
        "records_one_group": int(len(hits)), "sums_equal_numpy": ok,
        "wall_ms": {name: spread(v, 1e3) for name, v in t.items()},
        "accumulate_ms": {"one_group": spread(k["one_acc"]), "pairs": spread(k["pairs_acc"])},
        "select_ms": {"one_group": spread(k["one_sel"]), "pairs": spread(k["pairs_sel"])},
        "order_ms": {"one_group": spread(k["one_order"]), "pairs": spread(k["pairs_order"])},
        "k2_scan_ms": spread(k["scan"]),
        "accumulate_read_GBps": {"one_group": round(matrix_bytes / (acc_one * 1e-3) / 1e9, 1) if acc_one > 0 else None,
                                 "pairs": round(matrix_bytes / (acc_pairs * 1e-3) / 1e9, 1) if acc_pairs > 0 else None},
        "accumulate_faster_than_scan": bool(acc_one < scan and acc_pairs < scan),
        "reps": args.reps,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    b.close()
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
