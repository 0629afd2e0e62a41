"""GPU: filter fill through the C++17 host class (ClassicSearch::doc_bits / doc_fill / adjust: a compiled program, and
the command line tool built on it: `cobs_gpu_query doc-stats` and `--fpr-adjust`), against the numpy checker and the
Python mirror."""
import os
import subprocess

import pytest

from tests import cases, fill_check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cobs_amd", "cobs_gpu_query")


def _run(*args):
    assert os.path.exists(TOOL), "build cobs_amd/cobs_gpu_query first (make -C cobs_amd/csrc)"
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("fillcli")
    q = oracle.random_sequence(200, 77)
    pc = cases.make_compact(os.path.join(str(d), "a.cobs_compact"), 2 * 8 * 8 + 5, 8, [601, 97, 1301], 2, 31, 1, 0.3, 5,
                            planted={3: 1.0, 70: 0.9, 130: 0.5}, query=q)
    pk = cases.make_classic(os.path.join(str(d), "b.cobs_classic"), 77, 401, 1, 31, 1, 0.6, 6, planted={0: 1.0, 76: 0.7}, query=q)
    return pc, pk, q


def test_doc_stats(gpu_lib, files):
    pc, pk, _q = files
    for path in (pc, pk):
        ix = fill_check.read_index(path)
        bits = fill_check.bits_of_file(path)
        sigs = fill_check.doc_sigs(ix)
        fill, fpr = fill_check.doc_fill(path), fill_check.doc_fpr(path)
        page_docs = 8 * ix["page_size"] if ix["kind"] == "compact" else len(ix["names"])
        want = ["0\t%s\t%d\t%d\t%d\t%.6f\t%.6f" % (ix["names"][d], d // page_docs, sigs[d], bits[d], fill[d], fpr[d])
                for d in range(len(ix["names"]))]
        r = _run("doc-stats", path)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == want
        cut = sorted(fill)[len(fill) // 2]
        r = _run("doc-stats", path, "--fill-above", repr(cut))
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == [w for w, f in zip(want, fill) if f > cut] and 0 < len(r.stdout.splitlines()) < len(want)
    assert _run("doc-stats").returncode != 0


@pytest.mark.parametrize("extra,mode,z", [((), "error", 0), (("--findere", "3"), "error", 3),
                                          (("--invalid-bases", "skip"), "skip", 0),
                                          (("--invalid-bases", "skip", "--findere", "2", "--positions"), "skip", 2)])
def test_fpr_adjust_lines_equal_the_python_mirror(gpu_lib, files, tmp_path, extra, mode, z):
    pc, pk, q = files
    q = q.decode()
    queries = [q, q[20:120]] if mode == "error" else [q[:90] + "N" + q[91:], q[20:120]]
    qf = tmp_path / "q.fa"
    qf.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(queries)))
    s = gpu_lib.Search([pc, pk], findere=z, invalid_bases=mode)
    r = _run("-i", pc, "-i", pk, "-t", "0.3", "--fpr-adjust", "-f", str(qf), *extra)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    pos = 0
    for i, query in enumerate(queries):
        want = s.search_adjusted(query, 0.3, 0)
        assert lines[pos] == "*q%d\t%d" % (i, len(want)) and len(want) > 0
        for w, ln in zip(want, lines[pos + 1:pos + 1 + len(want)]):
            f = ln.split("\t")
            assert f[0] == w.doc_name and int(f[1]) == w.score
            assert f[-2:] == ["%.2f" % w.expected_fp, "%.2f" % w.adjusted], (ln, w)
            assert len(f) == (5 if "--positions" in extra else 4)
        pos += 1 + len(want)
    assert pos == len(lines)
    # the verbatim-query form
    r = _run("-i", pc, "-i", pk, "-t", "0.3", "--fpr-adjust", *[e for e in extra if e != "--positions"], queries[0])
    assert r.returncode == 0, r.stderr
    want = s.search_adjusted(queries[0], 0.3, 0)
    assert r.stdout.splitlines() == ["%s\t%d\t%.2f\t%.2f" % (w.doc_name, w.score, w.expected_fp, w.adjusted) for w in want]
    # the device list has no counterpart
    r = _run("-i", pc, "--sharded", "--fpr-adjust", queries[1])
    assert r.returncode != 0 and "--fpr-adjust" in r.stderr


_MIRROR_PROGRAM = r'''
#include <cstdio>
#include <string>
#include <vector>
#include "cobs_gpu_search.hpp"
// argv: compact classic query  ->  "bits f v...", "fill f v...", "adj name score expected adjusted", "refused <status>" lines
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    try {
        cobs_gpu::ClassicSearch s(std::vector<std::string>{argv[1], argv[2]});
        for (size_t f = 0; f < 2; ++f) {
            std::printf("bits %zu", f);
            for (uint64_t b : s.doc_bits(f)) std::printf(" %llu", (unsigned long long)b);
            std::printf("\nfill %zu", f);
            for (double v : s.doc_fill(f)) std::printf(" %.17g", v);
            std::printf("\n");
        }
        const std::string q = argv[3];
        std::vector<cobs_gpu::SearchResult> res;
        s.set_findere(2);
        s.search(q, res, 0.3, 0);
        const auto adj = s.adjust(res, q.size());
        for (size_t i = 0; i < res.size(); ++i)
            std::printf("adj %s %u %.17g %.17g\n", res[i].doc_name, res[i].score, adj[i].expected_fp, adj[i].adjusted);
        // a result that is not from this object
        std::vector<cobs_gpu::SearchResult> alien{cobs_gpu::SearchResult("doc_00000", 5)};
        try { s.adjust(alien, q.size()); std::printf("accepted\n"); }
        catch (const cobs_gpu::Error& e) { std::printf("refused %d\n", (int)e.status); }
        // under skip the valid positions are not at hand: refused without them, taken when passed
        s.set_invalid_bases(COBS_GPU_INVALID_SKIP);
        try { s.adjust(res, q.size()); std::printf("accepted\n"); }
        catch (const cobs_gpu::Error& e) { std::printf("refused %d\n", (int)e.status); }
        const std::vector<uint64_t> pos{100, 50};
        const auto adj2 = s.adjust(res, q.size(), &pos);
        std::printf("pos %.17g\n", res.empty() ? 0.0 : adj2[0].expected_fp / adj[0].expected_fp);
        // a shard holds part of the documents: doc_bits answers for its slots, doc_fill refuses
        cobs_gpu_options o{};
        o.struct_size = sizeof o;
        o.device = -1;
        o.shard_rank = 1;
        o.shard_count = 2;
        const char* path = argv[1];
        cobs_gpu_index* ix = nullptr;
        if (cobs_gpu_open(&path, 1, &o, &ix) != COBS_GPU_OK) return 3;
        cobs_gpu::ClassicSearch shard(ix);
        std::printf("shard %zu\n", shard.doc_bits(0).size());
        try { shard.doc_fill(0); std::printf("accepted\n"); }
        catch (const cobs_gpu::Error& e) { std::printf("refused %d\n", (int)e.status); }
    } catch (const cobs_gpu::Error& e) {
        std::printf("error %d %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
'''


def test_cpp_mirror_compiled(gpu_lib, files, tmp_path):
    """ClassicSearch::doc_bits / doc_fill / adjust from a compiled program: values against the checker and the Python
    mirror, and the refusals -- a foreign result, `skip` without the valid positions, doc_fill on a shard"""
    from cobs_amd import _capi
    pc, pk, q = files
    src = tmp_path / "fill_mirror.cpp"
    src.write_text(_MIRROR_PROGRAM)
    exe = str(tmp_path / "fill_mirror")
    lib_dir = os.path.join(ROOT, "cobs_amd")
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                         "-L", lib_dir, "-lcobs_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe, pc, pk, q.decode()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for f, path in enumerate((pc, pk)):
        bits = [ln.split()[2:] for ln in lines if ln.startswith("bits %d" % f)][0]
        fill = [ln.split()[2:] for ln in lines if ln.startswith("fill %d" % f)][0]
        assert [int(b) for b in bits] == fill_check.bits_of_file(path).tolist()
        assert [float(v) for v in fill] == fill_check.doc_fill(path)
    s = gpu_lib.Search([pc, pk], findere=2)
    want = s.search_adjusted(q, 0.3, 0)
    adj = [ln.split() for ln in lines if ln.startswith("adj ")]
    assert len(adj) == len(want) > 0
    for a, w in zip(adj, want):
        assert a[1] == w.doc_name and int(a[2]) == w.score
        assert abs(float(a[3]) - w.expected_fp) <= 1e-12 * abs(w.expected_fp)
        assert abs(float(a[4]) - w.adjusted) <= 1e-12 * abs(w.adjusted)
    rest = [ln for ln in lines if not ln.startswith(("bits", "fill", "adj "))]
    assert rest[0] == "refused %d" % _capi.ERR_ARG
    assert rest[1] == "refused %d" % _capi.ERR_UNSUPPORTED
    # expected_fp is linear in the positions: P of the first result's file in place of T - z
    f0 = s.search_hits([q], 0.3, 0)[0][0][0]
    T = len(q) - 31 + 1 - 2
    assert abs(float(rest[2].split()[1]) - (100, 50)[f0] / T) < 1e-12
    i = gpu_lib.Search(pc, shard_rank=1, shard_count=2).info(0)
    assert rest[3] == "shard %d" % int(i.slot_count) and 0 < int(i.slot_count) < int(i.counts_size)
    assert rest[4] == "refused %d" % _capi.ERR_UNSUPPORTED
