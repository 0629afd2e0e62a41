#!/usr/bin/env python3
"""scripts/findere_bench.py [ROUNDS] -- interleaved A/B of the scan kernel (K2) with findere z = 0 and z = 3 on ONE handle
of the C3 index (bench.c3_config(): compact, 100 000 documents, 8 sub-indexes):
  c3     the headline batch: 10 000 queries of 1000 terms, score rows (Batch.run)
  reads  40 000 reads of 100 bp on the same index (the multi-query scan), hits only at threshold 0.8 (Batch.run_hits)
z alternates inside every round (3 runs each, the last one's Batch.kernel_ms counts; round 0 is warm-up).  Prints the
median scan ms of both, the algorithmic bytes fraction of HBM peak (the same rows are gathered either way) and the
ratio z = 3 / z = 0."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import cobs_amd  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    cfg = bench.c3_config()
    s = cobs_amd.Search.synthetic(cfg["kind"], cfg["signature_sizes"], cfg["num_docs"], page_size=cfg["page_size"], seed=1)
    shapes = [("c3", 10000, 1000, lambda b: b.run(0.0)), ("reads100", 40000, 70, lambda b: b.run_hits(0.8))]
    for name, nq, kmers, run in shapes:
        b = cobs_amd.Batch(s)
        b.set_queries(bench.make_queries(nq, kmers))
        times = {0: [], 3: []}
        algo = {}
        for rnd in range(rounds + 1):
            for z in (0, 3):
                s.set_findere(z)
                for _ in range(3):
                    run(b)
                b.sync()
                ms = b.kernel_ms()["scan_ms"]
                algo[z] = b.stats()["algorithmic_bytes"]
                if rnd:
                    times[z].append(ms)
        s.set_findere(0)
        b.close()
        med = {z: statistics.median(t) for z, t in times.items()}
        for z in (0, 3):
            frac = algo[z] / (med[z] * 1e-3) / 1e9 / bench.HBM_PEAK_GBS
            print("%-9s z=%d  scan median %.3f ms  min %.3f  max %.3f  algorithmic bytes %d  frac %.3f" %
                  (name, z, med[z], min(times[z]), max(times[z]), algo[z], frac))
        print("%-9s ratio z=3 / z=0: %.3f  (%d rounds)" % (name, med[3] / med[0], rounds))
        sys.stdout.flush()
    s.close()


if __name__ == "__main__":
    main()
