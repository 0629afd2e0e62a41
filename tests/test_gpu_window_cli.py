"""GPU: cobs_gpu_query --window (ClassicSearch::search_window, the C++ mirror, through the tool) against
tests/window_check.py on one classic and one compact file, with --positions the printed bitmap and start, and the flag
conflicts."""
import os
import subprocess

import pytest

from tests import invalid_check as I
from tests import prevalence_check as V
from tests import window_check as B
from tests.test_gpu_weighted import SRC, _classic, _compact, _edge_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


def test_cli_and_cpp_mirror_agree_with_the_checker(gpu_lib, tmp_path):
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 300, 2003, 1, 31, 1)
    pb, fb = _compact(str(tmp_path / "b.cobs_compact"), 150, 4, [499, 601, 701, 557, 811], 2, 20, 2)
    paths, files = [pa, pb], [fa, fb]
    queries = _edge_queries(SRC, 31, 3, (1, 64, 200)) + [I.with_n(SRC[100:300], [90])]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, q.decode()) for i, q in enumerate(queries)))
    index_args = ["-i", paths[0], "-i", paths[1]]
    for z, mode, t, nr, W in ((0, "miss", 0.5, 0, 40), (3, "skip", 0.8, 5, 100)):
        rows = [B.results(files, q, z, W, t, nr, mode) for q in queries]
        assert sum(len(r) for r in rows) > 0
        fl = (["--findere", str(z)] if z else []) + ["--invalid-bases", mode, "-t", str(t)] + (["-l", str(nr)] if nr else [])
        r = subprocess.run([TOOL] + index_args + fl + ["-f", str(qf), "--window", str(W)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want = []
        for i, seg in enumerate(rows):
            want.append("*q%d\t%d" % (i, len(seg)))
            want += ["doc_%05d\t%d" % (d, sc) for (_f, d, sc) in seg]
        assert r.stdout.splitlines() == want
        # --positions: the bitmap of --positions and the first start of a window that reaches the score
        r = subprocess.run([TOOL] + index_args + fl + ["-f", str(qf), "--window", str(W), "--positions"], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want, moved = [], 0
        for i, seg in enumerate(rows):
            want.append("*q%d\t%d" % (i, len(seg)))
            wins = [V.windows(f, queries[i], z, mode) for f in files]
            for (f, d, sc) in seg:
                slot = int((files[f].doc_of_slot() == d).nonzero()[0][0])
                bits = wins[f][:, slot]
                best, start = B.best_window(bits, W)
                assert best == sc
                moved += int(start > 0)
                want.append("doc_%05d\t%d\t%s\t%d" % (d, sc, "".join("1" if b else "0" for b in bits), start))
        assert r.stdout.splitlines() == want and moved > 0
    # one file each, a verbatim query: the result lines only
    q = queries[2]
    for path, f in zip(paths, files):
        r = subprocess.run([TOOL, "-i", path, "--window", "64", "-t", "0.5", q.decode()], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want = ["doc_%05d\t%d" % (d, sc) for (_f, d, sc) in B.results([f], q, 0, 64, 0.5, 0)]
        assert r.stdout.splitlines() == want and want


def test_flag_conflicts_are_errors(gpu_lib, tmp_path):
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 40, 503, 1, 31, 1)
    sets = tmp_path / "sets.tsv"
    sets.write_text("doc_00000\ta\n")
    q = SRC[:100].decode()
    for extra in (["--hbm-budget", "1"], ["-d", "0,1"], ["--sharded"], ["--prevalence"], ["--weighted"], ["--coverage"],
                  ["--group", "2"], ["--sets", str(sets)], ["--sets", str(sets), "--sets-quorum", "0.5"],
                  ["--sets", str(sets), "--sets-profile"], ["--fpr-adjust"]):
        r = subprocess.run([TOOL, "-i", pa] + extra + ["--window", "50", q], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--window: not with" in r.stderr and r.stdout == "", (extra, r.stderr)
    for n in ("0", "4096"):
        r = subprocess.run([TOOL, "-i", pa, "--window", n, q], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--window: a number of positions, 1 .. 4095" in r.stderr and r.stdout == "", (n, r.stderr)
