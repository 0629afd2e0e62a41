"""GPU: cobs_gpu_query --best N|all and --best-by-name SEP line for line against the Python mirror (which
tests/test_gpu_best.py holds against the checker), the usage errors of the exclusive flags, and the C++17 mirror through
a small program (tests/cpp/best_api.cpp)."""
import os
import subprocess

import pytest

from tests import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


@pytest.fixture(scope="module")
def setup(gpu_lib, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("best_cli")
    src = oracle.random_sequence(1200, 13)
    path = str(d / "c.cobs_classic")
    cases.make_classic(path, 90, 1501, 1, 31, 1, 0.3, 3, planted={2: 1.0, 40: 1.0, 77: 0.8}, query=src)
    names = ["a_1", "a_2 second allele", "b_1", "c", "c", "d_x_1", "d_x_2", "d_y_1"]
    queries = [src[0:90], src[40:160], src[300:380], src[500:640], src[500:600], src[700:800], src[720:860], src[900:1000]]
    fa = d / "alleles.fa"
    fa.write_text("".join(">%s\n%s\n%s\n" % (n, q[:50].decode(), q[50:].decode()) for n, q in zip(names, queries)))
    return path, str(fa), [n.split()[0] for n in names], names, queries


def _text(s, labels, names, offsets, results):
    out = ""
    for g, rows in enumerate(results):
        out += "*%s\t%d\n" % (labels[g], len(rows))
        out += "".join("%s\t%s\t%d\t%d\t%d\n" % (r.doc_name, names[r.query], r.score, r.positions, r.ties) for r in rows)
    return out


def test_cli_best_is_the_python_mirror(gpu_lib, setup):
    path, fa, names, headers, queries = setup
    base = [TOOL, "-i", path, "-f", fa]
    s = gpu_lib.Search(path)
    cuts = {"3": [0, 3, 6, 8], "all": [0, 8], "_": [0, 2, 3, 4, 5, 7, 8]}
    labels = {"3": [headers[0], headers[3], headers[6]], "all": [headers[0]], "_": ["a", "b", "c", "c", "d_x", "d_y"]}
    for flag, arg, t, lim, z, mode in (("--best", "3", 0.8, 0, 0, "error"), ("--best", "all", 0.5, 5, 3, "error"),
                                       ("--best", "3", 0.0, 2, 0, "miss"), ("--best-by-name", "_", 0.8, 0, 1, "skip"),
                                       ("--best-by-name", "_", 0.0, 3, 0, "error")):
        r = subprocess.run(base + [flag, arg, "-t", str(t), "-l", str(lim), "--findere", str(z), "--invalid-bases", mode],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        s.set_findere(z)
        s.invalid_bases = mode
        want = s.search_best(queries, cuts[arg], t, lim)
        assert any(want) and r.stdout == _text(s, labels[arg], names, cuts[arg], want), (flag, arg, r.stdout[:300])
    s.close()


def test_cli_refuses_the_exclusive_flags(gpu_lib, setup):
    path, fa, _names, _headers, _queries = setup
    base = [TOOL, "-i", path, "-f", fa]
    for extra in (["--best", "3", "--group", "2"], ["--best", "3", "--weighted"], ["--best", "all", "--coverage"],
                  ["--best", "3", "--window", "20"], ["--best", "3", "--prevalence"], ["--best-by-name", "_", "--positions"],
                  ["--best", "3", "--fpr-adjust"], ["--best", "3", "--best-by-name", "_"], ["--best", "0"],
                  ["--best", "3", "--hbm-budget", "1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--best" in r.stderr and r.stdout == "", extra


def test_cpp_mirror(gpu_lib, setup, tmp_path):
    path, _fa, _names, _headers, queries = setup
    exe = str(tmp_path / "best_api")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "best_api.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "cobs_amd"), "-lcobs_gpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "cobs_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    s = gpu_lib.Search(path)
    for z, t, lim, step in ((0, 0.8, 0, 3), (3, 0.0, 4, 8), (1, 0.5, 0, 1)):
        r = subprocess.run([exe, str(z), str(t), str(lim), str(step), path] + [q.decode() for q in queries],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        s.set_findere(z)
        want = s.search_best(queries, group_size=step, threshold=t, num_results=lim)
        text = ""
        for g, rows in enumerate(want):
            text += "group %d %d\n" % (g, len(rows))
            text += "".join("%s\t%d\t%d\t%d\t%d\n" % (x.doc_name, x.query, x.score, x.positions, x.ties) for x in rows)
        assert any(want) and r.stdout == text, (z, t, lim, step)
    s.close()
