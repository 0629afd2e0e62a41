"""The prevalence checker (test infrastructure), on top of tests/findere_check.py, positions_check.py and invalid_check.py:
for every position of a query, how many REAL documents hold it.  Position p of n = T_f - z is set in a document when the
terms p .. p + z are all present there (FileBits.presence: all H bits of a term set in the document's column); the count
runs over the score slots that carry a document (doc_of_slot() >= 0) -- padding slots never count, whatever bits a file
holds there -- and, for one shard of several, over the slots [slot_begin, slot_begin + slot_count) only.  Under the
invalid-bases policies `miss` and `skip` a term that holds a character outside ACGT is absent (invalid_check.presence), so a
position whose window holds one reads 0.  No engine code in it."""
import numpy as np

from tests import invalid_check as I
from tests import positions_check as P


def windows(fb, q, z, mode="error"):
    """bool [n, slots]: position p set in the document of every score slot"""
    if mode == "error":
        return P._windows(fb, bytes(q), z)
    assert mode in I.MODES
    pres = I.presence(fb, q)
    n = max(pres.shape[0] - z, 0)
    win = np.ones((n, pres.shape[1]), dtype=bool)
    for j in range(z + 1):
        win &= pres[j:j + n]
    return win


def prevalence(fb, q, z, mode="error", slot_begin=0, slot_count=None):
    """uint32 [n]: the real documents (of the slot range) in which every position of q is set"""
    real = fb.doc_of_slot() >= 0
    if slot_count is not None:
        keep = np.zeros(len(real), dtype=bool)
        keep[slot_begin:slot_begin + slot_count] = True
        real = real & keep
    return windows(fb, q, z, mode)[:, real].sum(axis=1).astype(np.uint32)


def segments(files, queries, z, mode="error", ranges=None):
    """(offsets uint64 [nq * nfiles + 1], counts uint32) in the layout cobs_gpu_prevalence returns; ranges: per file
    (slot_begin, slot_count) of a shard, or None"""
    parts, offs = [], [0]
    for q in queries:
        for fi, fb in enumerate(files):
            b, c = ranges[fi] if ranges else (0, None)
            parts.append(prevalence(fb, q, z, mode, b, c))
            offs.append(offs[-1] + len(parts[-1]))
    counts = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    return np.array(offs, dtype=np.uint64), counts.astype(np.uint32)
