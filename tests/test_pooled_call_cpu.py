"""CPU: the host arithmetic of a pooled search call (cobs_amd/csrc/pooled_call.hpp: min_key, first_pool_cap,
real_documents / real_ranges, cut_passes, hand_out_lists) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer -- tests/host/pooled_call.cpp has its own main, no device code and needs no HIP header;
nothing that is loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pooled_call_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pooled_call")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # (the sanitizer runtimes linked statically: the program does not depend on what else the process loads)
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "host", "pooled_call.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "pooled_call ok" in out.stdout
