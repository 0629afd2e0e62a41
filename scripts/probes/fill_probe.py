#!/usr/bin/env python3
"""scripts/probes/fill_probe.py -- the arithmetic-free yardstick of the filter-fill kernel.

cobs_gpu_doc_bits_probe_ms launches fill_count_kernel<true> over the resident chunks of one file of an open handle: the
same grid, the same 16-byte loads over the same buffers, but one XOR per load instead of the carry-save counters and one
store per lane instead of the flush.  What it takes is what the loads alone cost on this box in this process; the
counting kernel is judged against it (scripts/fill_bench.py), not against a specification number.

    from scripts.probes.fill_probe import probe_ms
    ms = probe_ms(search, file_no=0)
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cobs_amd._capi import check  # noqa: E402


def probe_ms(search, file_no=0):
    """milliseconds (HIP events) of one load-only sweep over the resident chunks of file_no"""
    ms = C.c_double(0.0)
    check(search._lib.cobs_gpu_doc_bits_probe_ms(search._h, int(file_no), C.byref(ms)))
    return ms.value


if __name__ == "__main__":
    import bench
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    s = bench.make_index(bench.c3_config(scale), 0)
    for _ in range(5):
        print("%.3f ms" % probe_ms(s))
