#!/usr/bin/env python3
"""scripts/window_times.py -- what the window scan (cobs_gpu_search_window) costs beside the coverage scan and the findere
scan on the same batch.

The C3 procedural geometry with planted documents and the headline batch (10 000 x 1000-position queries cut from the
planted sequences) at threshold 0.8.  In one process, on one handle, alternating, several repetitions each (every
measured call follows an unmeasured call of its own kind): the stages of the window call (cobs_gpu_window_ms: K1, window
scan) at every W of --windows, and the two yardsticks, code the window call does not change: the coverage scan
(cobs_gpu_coverage_ms) and the plain scan of search_arrays at the same threshold (the handle's "scan" timer: the findere
scan with its threshold epilogue).  Then one batch of --long-queries queries of --long-kmers positions (random sequence
with a stretch of a planted sequence in the middle: the workload the call is for) at the last W.

Algorithmic row bytes of the window scan: TWO row streams -- positions x H x (z + 1) x row bytes per sub-index for the
incoming position and the same again for the outgoing one (the first w positions of a walk read the zero row instead).

All calls run at findere z (--findere, default 3), not at z = 0: the procedural filters are 30 % full, so at z = 0 a
random document holds a position with probability 0.3 and a thresholded call at a short window would return most of the
10^9 (query, document) pairs.  At z = 3 a random position is set with probability 0.3^4.
A text table on stdout, the same in --out (default profiles/window_times.txt).

    python scripts/window_times.py [--reps 3] [--queries 10000] [--kmers 1000] [--scale 1.0] [--threshold 0.8] [--findere 3]
                                   [--windows 31,255,1000] [--long-queries 100] [--long-kmers 20000] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def long_queries(plants, n, positions, stretch, findere, seed=23):
    """random sequences of `positions` positions with `stretch` positions of planted sequence q % n_seq in the middle"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for q in range(n):
        w = acgt[rs.randint(0, 4, size=positions + 30 + findere)].copy()
        text = np.frombuffer(plants[q % len(plants)][0], dtype=np.uint8)
        piece = text[:stretch + 30 + findere]
        off = (len(w) - len(piece)) // 2
        w[off:off + len(piece)] = piece
        out.append(w.tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--kmers", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--findere", type=int, default=3)
    ap.add_argument("--windows", default="31,255,1000")
    ap.add_argument("--long-queries", type=int, default=100)
    ap.add_argument("--long-kmers", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_times.txt"))
    args = ap.parse_args()
    windows = [int(w) for w in args.windows.split(",")]
    cfg = bench.c3_config(args.scale)
    plants = bench.planted_documents(cfg, args.kmers)
    cfg["plants"] = plants
    queries = bench.planted_queries(plants, args.queries, args.kmers)
    longs = long_queries(plants, args.long_queries, args.long_kmers, args.kmers, args.findere)
    s = bench.make_index(cfg, 0)
    s.set_findere(args.findere)
    win = {w: [] for w in windows}
    win_hash = []
    hits_w = {}
    cov, k2, lng = [], [], []
    hits_c = hits_k2 = hits_l = 0

    def window_call(qs, w):
        # every measured call follows an unmeasured call of its own kind: clocks and caches as in a stream of such calls
        s.search_window_arrays(qs, w, args.threshold, 0)
        s.window_ms()
        offs, _hits = s.search_window_arrays(qs, w, args.threshold, 0)
        t = s.window_ms()
        assert t["passes"] == 1, t               # (one run of one pass: the result buffer of the mirror was large enough)
        return t, int(offs[-1])

    for rep in range(args.reps):
        for w in windows:
            t, hits_w[w] = window_call(queries, w)
            win[w].append(t["scan_ms"])
            win_hash.append(t["hash_ms"])
        s.search_coverage_arrays(queries, args.threshold, 0)
        s.coverage_ms()
        offs, _hits = s.search_coverage_arrays(queries, args.threshold, 0)
        t = s.coverage_ms()
        assert t["passes"] == 1, t
        hits_c = int(offs[-1])
        cov.append(t["scan_ms"])
        s.search_arrays(queries, args.threshold, 0)
        s.timers(reset=True)
        offs, _hits = s.search_arrays(queries, args.threshold, 0)
        hits_k2 = int(offs[-1])
        k2.append(s.timers(reset=True)["scan"] * 1e3)
        t, hits_l = window_call(longs, windows[-1])
        lng.append(t["scan_ms"])
        print("rep %d: window scan %s ms, coverage scan %.3f ms, search_arrays scan %.3f ms, long batch %.3f ms" %
              (rep, " / ".join("%.3f" % win[w][-1] for w in windows), cov[-1], k2[-1], lng[-1]), flush=True)
    med = statistics.median
    row_bytes = cfg["page_size"] * len(cfg["signature_sizes"]) * cfg["num_hashes"]
    per_position = row_bytes * (args.findere + 1)

    def line(name, v):
        return "%-28s %9.3f  [%9.3f .. %9.3f]" % (name, med(v), min(v), max(v))

    lines = ["# scripts/window_times.py: C3 procedural (scale %g), %d queries x %d k-mers from planted sequences, threshold %g, "
             "findere %d, %d repetitions (median [min .. max], ms)" % (args.scale, len(queries), args.kmers, args.threshold, args.findere, args.reps),
             "# all calls at findere %d; the yardsticks are the coverage scan and search_arrays' scan (the findere scan) on the same batch"
             % args.findere,
             line("window hash_ms", win_hash)]
    for w in windows:
        positions = len(queries) * args.kmers
        out_positions = len(queries) * max(args.kmers - w, 0)
        algo = (positions + out_positions) * per_position
        lines.append(line("window scan_ms W=%d" % w, win[w]) + "  hits %d; %.3e algorithmic row bytes (incoming %.3e + outgoing %.3e), %.3f TB/s;"
                     " x %.3f the coverage scan, x %.3f the search_arrays scan" %
                     (hits_w[w], algo, positions * per_position, out_positions * per_position, algo / med(win[w]) / 1e9,
                      med(win[w]) / med(cov), med(win[w]) / med(k2)))
    lines += [line("coverage scan_ms", cov) + "  hits %d" % hits_c,
              line("scan of search_arrays", k2) + "  hits %d" % hits_k2]
    positions = len(longs) * args.long_kmers
    out_positions = len(longs) * max(args.long_kmers - windows[-1], 0)
    algo = (positions + out_positions) * per_position
    lines.append(line("long batch scan_ms W=%d" % windows[-1], lng) + "  %d queries x %d positions, %d of them planted; hits %d; "
                 "%.3e algorithmic row bytes, %.3f TB/s" % (len(longs), args.long_kmers, args.kmers, hits_l, algo, algo / med(lng) / 1e9))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    s.close()


if __name__ == "__main__":
    main()
