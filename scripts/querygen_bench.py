"""Measures generate-queries (cobs_gpu_generate_queries) on the corpus of scripts/construct_bench.py.

    python scripts/querygen_bench.py [--docs 256] [--doc-mb 4] [--dir /tmp/cobs_querygen_bench]
                                     [--positive 10000] [--negative 1000000] [--size 100]

Writes the FASTA documents construct_bench.py writes (same sizes, same seed), then times, on one GPU
at k = 31 (best of --reps):
  positives  -p only: the documents holding a positive are read and their terms numbered
  true_neg   -p, -n NEG of SIZE bases and -N: every document read, every ACGT term probed
  canonical  the same with --canonical
Each gives wall seconds, text GB/s (term text scanned / wall) and the kernel ms the library
reports.  One JSON line.  `rocprofv3 --kernel-trace --stats` around this command gives the kernels'
own times."""
import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--doc-mb", type=float, default=4.0)
    ap.add_argument("--dir", default="/tmp/cobs_querygen_bench")
    ap.add_argument("--positive", type=int, default=10000)
    ap.add_argument("--negative", type=int, default=1000000)
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--keep", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401
    import cobs_amd
    from construct_bench import write_docs

    docdir = os.path.join(a.dir, "docs")
    t0 = time.time()
    write_docs(docdir, a.docs, int(a.doc_mb * 1e6))
    out = {"docs": a.docs, "generate_s": round(time.time() - t0, 2), "k": 31, "positive": a.positive,
           "negative": a.negative, "size": a.size}
    dl = cobs_amd.DocumentList(docdir)
    out["terms"] = sum(d.num_terms(31) for d in dl)
    cobs_amd.generate_queries(dl, positive=10, seed=1, device=0)            # warm-up: HIP context, pinned pools
    runs = {"positives": dict(positive=a.positive),
            "true_neg": dict(positive=a.positive, negative=a.negative, size=a.size, true_negatives=True),
            "canonical": dict(positive=a.positive, negative=a.negative, size=a.size, true_negatives=True,
                              canonical=True)}
    for name, kw in runs.items():
        best = None
        for rep in range(a.reps):
            t0 = time.time()
            got = cobs_amd.generate_queries(dl, seed=42 + rep, device=0, **kw)
            dt = time.time() - t0
            if best is None or dt < best[0]:
                best = (dt, got.stats, len(got))
        dt, st, n = best
        out[name] = {"wall_s": round(dt, 3), "text_GB_per_s": round(st["text_bytes"] / dt / 1e9, 2),
                     "kernel_ms": round(st["kernel_ms"], 2), "documents_read": st["documents_read"],
                     "text_bytes": st["text_bytes"], "terms_probed": st["terms_probed"],
                     "negatives_removed": st["negatives_removed"], "queries": n}
    print(json.dumps(out))
    if not a.keep:
        shutil.rmtree(a.dir, ignore_errors=True)


if __name__ == "__main__":
    main()
