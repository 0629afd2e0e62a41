#!/usr/bin/env python3
"""scripts/invalid_bases_bench.py [OUT] -- K1 (hash_ms), K2 (scan_ms) and the step under every invalid-bases policy on ONE
handle of the C3 index with the benchmark's headline batch (10 000 queries of 1000 k-mers), at thresholds 0 and 0.8 (under
`skip` the latter adds skip_thresholds_kernel), with clean queries and with two Ns in one read of twenty.  One JSON line
per (queries, policy, threshold, repetition); the lines also go to OUT (default profiles/invalid_bases_k1.txt)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import cobs_amd  # noqa: E402
cfg = bench.c3_config(1.0)
cfg["num_hashes"] = 1
s = bench.make_index(cfg, 0)
clean = bench.make_queries(10000, 1000, seed=42)
rng = np.random.default_rng(1)
dirty = []
for i, q in enumerate(clean):
    b = bytearray(q if isinstance(q, (bytes, bytearray)) else q.encode())
    if i % 20 == 0:                      # one read in twenty holds two Ns
        for o in rng.integers(0, len(b), size=2):
            b[int(o)] = ord("N")
    dirty.append(bytes(b))
out = []
for label, qs in (("clean", clean), ("n_in_5pct", dirty)):
    for rep in range(2):
        for mode in ("error", "miss", "skip"):
            if label != "clean" and mode == "error":
                continue
            s.invalid_bases = mode
            for thr in (0.0, 0.8):
                b = cobs_amd.Batch(s)
                b.set_queries(qs)
                for _ in range(5):
                    b.run(thr)
                b.sync(); b.kernel_ms()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    b.run(thr)
                b.sync()
                dt = (time.perf_counter() - t0) / 20 * 1e3
                ms = b.kernel_ms()
                rec = {"queries": label, "mode": mode, "threshold": thr, "rep": rep, "hash_ms": round(ms["hash_ms"], 4),
                       "scan_ms": round(ms["scan_ms"], 4), "step_ms": round(dt, 4)}
                print(json.dumps(rec), flush=True)
                out.append(rec)
                b.close()
open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "invalid_bases_k1.txt"), "w").write("\n".join(json.dumps(r) for r in out) + "\n")
