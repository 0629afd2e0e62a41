"""CPU: the shape-class selection of the self-hashing scan (geometry.cpp: scan_geometry, tile_sub_indexes, self_hash_fits,
self_hash_shape, pass_self_hash) as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer --
tests/host/self_hash_select.cpp has its own main and no device code; nothing that is loaded into Python runs under a
sanitizer."""
import glob
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include():
    for d in [os.environ.get("ROCM_PATH", ""), "/opt/rocm"] + sorted(glob.glob("/opt/rocm-*")):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(d, "include")
    raise AssertionError("no HIP headers found (ROCM_PATH)")


def test_selection_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "self_hash_select")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # (the sanitizer runtimes linked statically: the program does not depend on what else the process loads)
                           "-static-libasan", "-static-libubsan",
                           "-D__HIP_PLATFORM_AMD__", "-I" + _hip_include(), "-I" + os.path.join(ROOT, "cobs_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "self_hash_select.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "self_hash_select ok" in out.stdout
