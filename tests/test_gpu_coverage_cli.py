"""GPU: cobs_gpu_query --coverage (ClassicSearch::search_coverage, the C++ mirror, through the tool) against
tests/coverage_check.py on one classic and one compact file, and the flag conflicts."""
import os
import subprocess

import pytest

from tests import coverage_check as G
from tests import invalid_check as I
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
    for z, mode, t, nr in ((0, "miss", 0.3, 0), (3, "skip", 0.8, 5)):
        rows = [G.results(files, q, z, t, nr, mode) for q in queries]
        assert sum(len(r) for r in rows) > 0
        s = gpu_lib.Search(paths, findere=z, invalid_bases=mode)
        offs, hits = s.search_coverage_arrays(queries, t, nr)
        got = hits.tolist()
        assert [got[int(offs[i]):int(offs[i + 1])] for i in range(len(queries))] == rows
        s.close()
        fl = (["--findere", str(z)] if z else []) + ["--invalid-bases", mode, "-t", str(t)] + (["-l", str(nr)] if nr else [])
        r = subprocess.run([TOOL] + index_args + fl + ["-f", str(qf), "--coverage"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want = []
        for i, seg in enumerate(rows):
            want.append("*q%d\t%d" % (i, len(seg)))
            want += ["doc_%05d\t%d" % (d, sc) for (_f, d, sc) in seg]
        assert r.stdout.splitlines() == want
    # one file each, a verbatim query: the result lines only
    q = queries[2]
    for path, f in zip(paths, files):
        r = subprocess.run([TOOL, "-i", path, "--coverage", "-t", "0.3", q.decode()], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want = ["doc_%05d\t%d" % (d, sc) for (_f, d, sc) in G.results([f], q, 0, 0.3, 0)]
        assert r.stdout.splitlines() == want and want


def test_flag_conflicts_are_errors(gpu_lib, tmp_path):
    pa, fa = _classic(str(tmp_path / "a.cobs_classic"), 40, 503, 1, 31, 1)
    sets = tmp_path / "sets.tsv"
    sets.write_text("doc_00000\ta\n")
    q = SRC[:100].decode()
    for extra in (["--hbm-budget", "1"], ["-d", "0,1"], ["--sharded"], ["--prevalence"], ["--weighted"], ["--group", "2"],
                  ["--sets", str(sets)], ["--positions"], ["--fpr-adjust"]):
        r = subprocess.run([TOOL, "-i", pa] + extra + ["--coverage", q], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--coverage: not with" in r.stderr and r.stdout == "", (extra, r.stderr)
