"""The filter-fill checker (test infrastructure): a plain numpy restatement of cobs_gpu_doc_bits and of the FPR
adjustment.  bits(f, d) = the rows of d's sub-index whose bit d % 8 of byte d / 8 is set; the matrices are read from
the index FILE with the parser below (the byte layout oracle/construct.py's writers produce, i.e. the reference's
cobs/file/{classic,compact}_index_header.cpp), or handed over as arrays (rows read back from the device).  Shares no
code with cobs_amd/.
"""
import math
import struct

import numpy as np


def read_index(path):
    """-> dict(kind, term_size, canonicalize, num_hashes, page_size, names, sigs, mats): mats[p] = uint8 [S_p, row bytes]
    of sub-index p (classic: one matrix of ceil(D / 8)-byte rows)"""
    raw = open(path, "rb").read()
    if raw[:18] == b"COBS:CLASSIC_INDEX":
        _ver, k, canon, ndocs, sig, nh = struct.unpack_from("<IIBIQQ", raw, 18)
        pos = 18 + struct.calcsize("<IIBIQQ")
        names = []
        for _ in range(ndocs):
            e = raw.index(b"\n", pos)
            names.append(raw[pos:e].decode())
            pos = e + 1
        assert raw[pos:pos + 13] == b"CLASSIC_INDEX"
        pos += 13
        row = (ndocs + 7) // 8
        m = np.frombuffer(raw, dtype=np.uint8, count=sig * row, offset=pos).reshape(sig, row)
        return dict(kind="classic", term_size=k, canonicalize=canon, num_hashes=nh, page_size=0, names=names, sigs=[sig], mats=[m])
    assert raw[:18] == b"COBS:COMPACT_INDEX", "not a COBS index"
    _ver, k, canon, nparams, ndocs, page_size = struct.unpack_from("<IIBIIQ", raw, 18)
    pos = 18 + struct.calcsize("<IIBIIQ")
    params = []
    for _ in range(nparams):
        params.append(struct.unpack_from("<QQ", raw, pos))
        pos += 16
    names = []
    for _ in range(ndocs):
        e = raw.index(b"\n", pos)
        names.append(raw[pos:e].decode())
        pos = e + 1
    pos += (page_size - ((pos + 13) % page_size)) % page_size
    assert raw[pos:pos + 13] == b"COMPACT_INDEX"
    pos += 13
    mats = []
    for s, _h in params:
        mats.append(np.frombuffer(raw, dtype=np.uint8, count=s * page_size, offset=pos).reshape(s, page_size))
        pos += s * page_size
    assert len({h for _s, h in params}) == 1
    return dict(kind="compact", term_size=k, canonicalize=canon, num_hashes=params[0][1], page_size=page_size, names=names,
                sigs=[s for s, _h in params], mats=mats)


def bits_of_mats(mats):
    """uint64 [score slots of the file]: per sub-index the column sums of its unpacked bits, in slot order"""
    return np.concatenate([np.unpackbits(np.ascontiguousarray(m), axis=1, bitorder="little").sum(axis=0, dtype=np.uint64)
                           for m in mats])


def bits_of_file(path):
    return bits_of_mats(read_index(path)["mats"])


def doc_sigs(ix):
    """S_p of the sub-index of every real document"""
    n = len(ix["names"])
    if ix["kind"] == "classic":
        return np.full(n, ix["sigs"][0], dtype=np.uint64)
    return np.array(ix["sigs"], dtype=np.uint64)[np.arange(n) // (8 * ix["page_size"])]


def doc_fill(path):
    ix = read_index(path)
    n = len(ix["names"])
    return [int(b) / int(s) for b, s in zip(bits_of_mats(ix["mats"])[:n], doc_sigs(ix))]


def doc_fpr(path):
    H = read_index(path)["num_hashes"]
    return [f ** H for f in doc_fill(path)]


def adjust(s, P, bits, sig, H, z=0):
    """the issue's table, in Python floats (libm): -> dict(fill, fpr, q, expected_fp, adjusted)"""
    fill = bits / sig
    fpr = math.pow(fill, H)
    q = math.pow(fpr, z + 1)
    expected = P * q
    adjusted = 0.0 if q >= 1.0 else max(0.0, (s - expected) / (1.0 - q))
    return dict(fill=fill, fpr=fpr, q=q, expected_fp=expected, adjusted=adjusted)
