"""The positions checker (test infrastructure), on top of tests/findere_check.py: which positions of a query are set in ONE
document.  Position p of n = T_f - z is set when the terms p .. p + z are all present in the document (FileBits.presence:
all H bits of a term set in the document's column); the words pack position p into bit p % 64 of word p // 64.  The
popcount of a pair's positions is the score tests/findere_check.py's results() gives that pair (under the policies `miss`
and `skip`: the score tests/invalid_check.py's results() gives it)."""
import functools

import numpy as np


@functools.lru_cache(maxsize=4)
def _windows(fb, q, z):
    """bool [n, slots]: position p set in the document of every score slot"""
    P = fb.presence(q)
    n = max(P.shape[0] - z, 0)
    win = np.ones((n, P.shape[1]), dtype=bool)
    for j in range(z + 1):
        win &= P[j:j + n]
    return win


@functools.lru_cache(maxsize=4)
def _windows_under(fb, q, z, mode):
    """_windows under the invalid-bases policies `miss` and `skip`: a term that holds a character outside ACGT is absent
    (invalid_check.presence), so a position whose window holds one is not set"""
    from tests import invalid_check as I
    assert mode in I.MODES
    P = I.presence(fb, q)
    n = max(P.shape[0] - z, 0)
    win = np.ones((n, P.shape[1]), dtype=bool)
    for j in range(z + 1):
        win &= P[j:j + n]
    return win


def positions(files, q, z, file_no, doc, mode="error"):
    """bool [n]: the positions of query q set in document `doc` of file `file_no` (mode: the invalid-bases policy)"""
    fb = files[file_no]
    slots = np.nonzero(fb.doc_of_slot() == doc)[0]
    assert len(slots) == 1, (doc, slots)
    win = _windows(fb, bytes(q), z) if mode == "error" else _windows_under(fb, bytes(q), z, mode)
    return win[:, int(slots[0])]


def pack(pos):
    """bool [n] -> uint64 [ceil(n / 64)], bits >= n zero"""
    n = len(pos)
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = pos
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def unpack(words, n):
    """uint64 words -> bool [n]"""
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8)).sum())
