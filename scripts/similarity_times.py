#!/usr/bin/env python3
"""scripts/similarity_times.py -- what one panel of cobs_gpu_doc_shared_bits costs, beside the filter-fill sweep.

The C3 geometry of bench.py as a resident procedural index (8 sub-indexes of 12 544 documents).  In one process: the
filter-fill sweep of the whole file (cobs_gpu_doc_bits_ms, the library's HIP events) and, on one sub-index (--page), panels
of 8 references of three fills: the procedural index's own (0.297, its generator's fixed density and so the sparsest
reference this geometry offers; a sparser one, such as 0.1, is NOT measured here) and about 0.5 and 0.9, reached by planting
random text on top (cobs_gpu_similarity_ms: the extraction of the references' bits and the sweep, HIP events).
Reported: milliseconds, TB/s of index bytes, the ratio of a panel's sweep to the fill kernel per byte -- per panel and per reference -- and the
projected time of `doc-similarity --all-pairs` over one sub-index (12 544 / 8 panels).  Text on stdout and in --out.

    python scripts/similarity_times.py [--scale 1.0] [--page 3] [--reps 5] [--out profiles/similarity_times.txt]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

M = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--page", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_times.txt"))
    args = ap.parse_args()
    cfg = bench.c3_config(args.scale)
    s = bench.make_index(cfg, 0)
    info = s.info(0)
    per = 8 * int(info.page_size)
    S = s.signature_size(0, args.page)
    d0 = args.page * per
    lines = ["C3 geometry x %g: sub-index %d, %d rows x %d bytes = %.3f GB" % (args.scale, args.page, S, per // 8, S * (per // 8) / 1e9)]
    # references of three fills: as generated (BASE), and with the k-mers planted that lift BASE to f -- each of n random
    # k-mers sets one bit (one hash function), so 1 - f = (1 - BASE) * exp(-n / S)
    BASE = 0.297
    groups = []
    for g, f in enumerate((None, 0.5, 0.9)):
        docs = [d0 + 8 * g + j for j in range(M)]
        if f is not None:
            n = int(-math.log((1.0 - f) / (1.0 - BASE)) * S)
            text = bench.make_queries(1, n + 30, seed=100 + g)[0]
            s.plant(text, docs, 1000, salt=g)
        groups.append(docs)
    # the fill sweep of the whole file (also gives the references' fills)
    fill_ms, fill_bytes = [], 0
    for rep in range(args.reps + 1):
        s.plant(bench.make_queries(1, 40, seed=7)[0], [0], 1000, salt=1000 + rep)      # drops the cached counts
        b = s.doc_bits_ms()
        bits = s.doc_bits()
        a = s.doc_bits_ms()
        if rep:
            fill_ms.append(a["kernel_ms"] - b["kernel_ms"])
            fill_bytes = a["bytes_read"] - b["bytes_read"]
    fm = statistics.median(fill_ms)
    fill_rate = fill_bytes / fm / 1e9          # TB/s
    lines.append("fill sweep (whole file, %.3f GB): %.3f ms median of %d, %.2f TB/s" % (fill_bytes / 1e9, fm, args.reps, fill_rate))
    for docs in groups:
        fills = [int(bits[d]) / S for d in docs]
        ext, swp, nbytes = [], [], 0
        for rep in range(args.reps + 1):
            s.similarity_ms()
            s.doc_shared_bits(docs)
            t = s.similarity_ms()
            assert t["sweeps"] == 1
            if rep:
                ext.append(t["extract_ms"])
                swp.append(t["sweep_ms"])
                nbytes = t["bytes_read"]
        e, w = statistics.median(ext), statistics.median(swp)
        rate = nbytes / w / 1e9
        ratio = fill_rate / rate
        pairs_ms = (per / M) * (e + w)
        lines.append("panel of %d references of measured fill %.3f..%.3f: ref_rows %.3f ms, sweep %.3f ms = %.2f TB/s; "
                     "sweep / fill per byte: %.2f per panel, %.3f per reference; all pairs of the sub-index (%d panels): %.2f s"
                     % (M, min(fills), max(fills), e, w, rate, ratio, ratio / M, per // M, pairs_ms / 1e3))
    lines.append("not measured: references sparser than the generator's density (fill 0.1), the only case in which whole blocks of "
                 "8 rows are skipped often")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
