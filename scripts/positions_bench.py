#!/usr/bin/env python
"""Cost of Search.hit_positions beside the search that produced the hits.

The procedural C3 index with planted documents and the batch of `bench.py --full`'s end_to_end at threshold 0.8
(10 000 queries of 1000 k-mers with hits): wall time of the search_arrays call and of the hit_positions call over its
hits, in the same process, several repetitions each; the presence kernel's and K1's milliseconds from the library's
event timers (Search.positions_ms).  The figure of merit is the ratio positions : search.  One JSON line on stdout,
the same in --out (default profiles/positions_bench.json).

    python scripts/positions_bench.py [--queries 10000] [--kmers 1000] [--reps 7] [--findere 0] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--findere", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "positions_bench.json"))
    args = ap.parse_args()

    cfg = bench.c3_config(args.scale)
    cfg["plants"] = bench.planted_documents(cfg, args.kmers)
    s = bench.make_index(cfg, 0)
    s.set_findere(args.findere)
    queries = bench.planted_queries(cfg["plants"], args.queries, args.kmers)

    t_search, t_pos, k_presence, k_hash = [], [], [], []
    offs = hits = bo = bits = None
    for rep in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        offs, hits = s.search_arrays(queries, args.threshold, 0)
        t1 = time.perf_counter()
        s.positions_ms()
        t2 = time.perf_counter()
        bo, bits = s.hit_positions(queries, offs, hits)
        t3 = time.perf_counter()
        ms = s.positions_ms()
        if rep >= args.warmup:
            t_search.append(t1 - t0)
            t_pos.append(t3 - t2)
            k_presence.append(ms["presence_ms"])
            k_hash.append(ms["hash_ms"])
    # the built-in self-check: the popcount of every hit's words is its score
    pc = np.add.reduceat(np.unpackbits(bits.view(np.uint8)).reshape(-1, 64).sum(axis=1), bo[:-1].astype(np.int64)) \
        if len(hits) else np.zeros(0)
    ok = bool(len(hits)) and bool(np.array_equal(pc.astype(np.uint64), hits["score"].astype(np.uint64)))

    def spread(v, scale=1.0):
        return {"median": round(statistics.median(v) * scale, 4), "min": round(min(v) * scale, 4), "max": round(max(v) * scale, 4)}

    lookups = int(sum((len(queries[i]) - cfg["term_size"] + 1) * int(offs[i + 1] - offs[i]) for i in range(len(queries))))
    med_k = statistics.median(k_presence)
    out = {
        "name": "positions_bench", "queries": len(queries), "kmers": args.kmers, "threshold": args.threshold,
        "findere": args.findere, "hits": int(len(hits)), "words": int(len(bits)), "popcount_equals_score": ok,
        "search_arrays_ms": spread(t_search, 1e3), "hit_positions_ms": spread(t_pos, 1e3),
        "ratio_positions_to_search": round(statistics.median(t_pos) / statistics.median(t_search), 4),
        "presence_kernel_ms": spread(k_presence), "k1_ms": spread(k_hash),
        # one byte of one row per (pair, term, hash): the USEFUL bytes; what the memory system moves per look-up is a
        # whole sector -- that figure comes from a counter run, not from here
        "lookups": lookups * cfg["num_hashes"],
        "useful_GBps": round(lookups * cfg["num_hashes"] / (med_k * 1e-3) / 1e9, 2) if med_k > 0 else None,
        "lookups_per_s": round(lookups * cfg["num_hashes"] / (med_k * 1e-3), 0) if med_k > 0 else None,
        "reps": args.reps,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
