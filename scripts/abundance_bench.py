"""Measures index construction with the k-mer abundance cutoff (min_count) beside the default path.

    python scripts/abundance_bench.py [--docs 64] [--doc-mb 4] [--repeat 2] [--reps 3] [--out profiles/abundance_bench.json]

The corpus is that of scripts/construct_bench.py (FASTA documents of random bases, 80-column lines);
with --repeat R every document holds its sequence R times as R records, so that a cutoff c <= R
keeps (nearly) every term and c > R none -- random bases alone hold no 31-mer twice.  For
c = 1, 2, 3 the documents are built into a resident handle (wall time, best and all of --reps) and
once into a file, whose set bits say what was kept: a document's column holds one bit per distinct
kept term (num_hashes = 1, less hash collisions).  Kernel times are not taken here: run this
command under `rocprofv3 --kernel-trace --stats` (abundance_count_kernel, abundance_emit_kernel,
build_kernel, pack_bytemap_kernel)."""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=64)
    ap.add_argument("--doc-mb", type=float, default=4.0)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/cobs_abundance_bench")
    ap.add_argument("--batch-mb", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abundance_bench.json"))
    a = ap.parse_args()
    import torch  # noqa: F401
    import cobs_amd
    from construct_bench import write_docs
    from oracle import construct as K

    base = os.path.join(a.dir, "base")
    docdir = os.path.join(a.dir, "docs")
    write_docs(base, a.docs, int(a.doc_mb * 1e6 / a.repeat))
    os.makedirs(docdir, exist_ok=True)
    for fn in sorted(os.listdir(base)):
        raw = open(os.path.join(base, fn), "rb").read()
        with open(os.path.join(docdir, fn), "wb") as f:
            for _ in range(a.repeat):
                f.write(raw)
    dl = cobs_amd.DocumentList(docdir)
    terms = sum(d.num_terms(31) for d in dl)
    out = {"docs": a.docs, "repeat": a.repeat, "file_bytes": sum(os.path.getsize(d.path) for d in dl),
           "total_occurrences": terms, "text_batch_mb": a.batch_mb or 256, "runs": {}}
    for c in (1, 2, 3):
        p = cobs_amd.ClassicIndexParameters()
        p.false_positive_rate, p.clobber, p.min_count, p.text_batch_bytes = 0.3, True, c, a.batch_mb << 20
        cobs_amd.build_search(list=dl, index_params=p).close()          # warm-up: context, pools, the table
        walls = []
        for _ in range(a.reps):
            t0 = time.time()
            s = cobs_amd.build_search(list=dl, index_params=p)
            walls.append(round(time.time() - t0, 4))
            s.close()
        idx = os.path.join(a.dir, "c%d.cobs_classic" % c)
        t0 = time.time()
        cobs_amd.classic_construct(list=dl, out_file=idx, index_params=p)
        file_s = round(time.time() - t0, 4)
        m = K.read_classic(idx)[5]
        bits = int(np.unpackbits(m).sum())
        out["runs"]["min_count_%d" % c] = {
            "resident_wall_s": walls, "resident_best_s": min(walls), "file_wall_s": file_s,
            "occurrences_per_s_best": round(terms / min(walls)), "index_bits_set": bits,
            "kept_occurrences_estimate": bits * (a.repeat if c <= a.repeat else 1)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    shutil.rmtree(a.dir, ignore_errors=True)


if __name__ == "__main__":
    main()
