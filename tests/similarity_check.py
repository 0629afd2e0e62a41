"""The document-similarity checker (test infrastructure): a plain numpy restatement of cobs_gpu_doc_shared_bits and of
cobs_gpu_jaccard_estimate.  shared(a, b) of one sub-index = the rows in which documents a and b both have their bit set;
the matrices come as fill_check.read_index delivers them (uint8 [S_p, row bytes], bit d % 8 of byte d / 8 = document d).
Shares no code with cobs_amd/.
"""
import math

import numpy as np

from tests import fill_check


def unpack(m):
    """uint8 [S, row bytes] -> uint64 0/1 [S, 8 * row bytes], little bit order: column d = score slot d of the sub-index"""
    return np.unpackbits(np.ascontiguousarray(m), axis=1, bitorder="little").astype(np.uint64)


def shared_of_mat(m, refs):
    """uint64 [len(refs), slots]: row i = shared(refs[i], d) for every slot d of the sub-index (refs are slots of it)"""
    cols = unpack(m)
    return cols[:, list(refs)].T @ cols


def page_docs(ix):
    """score slots per sub-index"""
    return ix["mats"][0].shape[1] * 8


def shared_of_index(ix, refs):
    """what Search.doc_shared_bits(refs) returns for an index read by fill_check.read_index: one uint64 array per
    reference (file-level document numbers), the slots of the reference's own sub-index"""
    per = page_docs(ix)
    out = []
    for r in refs:
        p, s = divmod(int(r), per)
        out.append(shared_of_mat(ix["mats"][p], [s])[0])
    return out


def shared_of_file(path, refs):
    return shared_of_index(fill_check.read_index(path), refs)


def n_of(t, sig, H):
    return -(sig / H) * math.log1p(-t / sig)


def estimate(sig, H, a, b, c):
    """-> (bit_jaccard, jaccard, containment_a_in_b, containment_b_in_a, n_inter), in Python floats (libm)"""
    t_or = a + b - c
    bj = c / t_or if t_or else 0.0
    if t_or == sig:
        nan = float("nan")
        return (bj, nan, nan, nan, nan)
    na, nb, nu = n_of(a, sig, H), n_of(b, sig, H), n_of(t_or, sig, H)
    inter = max(0.0, na + nb - nu)
    return (bj, inter / nu if nu > 0 else 0.0, min(1.0, inter / na) if na > 0 else 0.0,
            min(1.0, inter / nb) if nb > 0 else 0.0, inter)


def reaches(j, min_jaccard):
    """the one threshold rule: min_jaccard <= 0 keeps every pair; a positive one keeps the pairs whose estimate reaches it,
    so a NaN estimate (a saturated filter) passes no threshold"""
    return not min_jaccard > 0 or j >= min_jaccard


def similar(ix, ref, min_jaccard=0.0, num_results=0):
    """what Search.similar_documents returns: the real documents of ref's sub-index but ref, (name, jaccard,
    containment_ref_in_doc, containment_doc_in_ref, shared), estimate descending then document; NaN estimates last, by
    bit_jaccard"""
    per = page_docs(ix)
    p, s = divmod(int(ref), per)
    cols = unpack(ix["mats"][p])
    bits = cols.sum(axis=0, dtype=np.uint64)
    sh = cols[:, s] @ cols
    sig, H, names = ix["sigs"][p], ix["num_hashes"], ix["names"]
    rows = []
    for t in range(min(per, len(names) - p * per)):
        d = p * per + t
        if d == ref:
            continue
        bj, j, cab, cba, _n = estimate(sig, H, int(bits[s]), int(bits[t]), int(sh[t]))
        nan = j != j
        if not reaches(j, min_jaccard):
            continue
        rows.append(((nan, -(bj if nan else j), d), (names[d], j, cab, cba, int(sh[t]))))
    rows.sort(key=lambda r: r[0])
    out = [r for _k, r in rows]
    return out[:num_results] if num_results else out


def all_pairs(ix, min_jaccard):
    """every unordered pair (a < b) of real documents of one sub-index whose estimated Jaccard reaches min_jaccard,
    sub-index by sub-index in (a, b) order: (a, b, sub-index, shared, bit_jaccard, jaccard, c_a_in_b, c_b_in_a)"""
    per = page_docs(ix)
    names = ix["names"]
    out = []
    for p, m in enumerate(ix["mats"]):
        cols = unpack(m)
        live = min(per, len(names) - p * per)
        bits = cols.sum(axis=0, dtype=np.uint64)
        sh = cols[:, :live].T @ cols[:, :live]
        for s in range(live):
            for t in range(s + 1, live):
                bj, j, cab, cba, _n = estimate(ix["sigs"][p], ix["num_hashes"], int(bits[s]), int(bits[t]), int(sh[s, t]))
                if reaches(j, min_jaccard):
                    out.append((p * per + s, p * per + t, p, int(sh[s, t]), bj, j, cab, cba))
    return out
