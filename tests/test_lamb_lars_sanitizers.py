"""The layer-wise optimizers' CPU code under sanitizers: csrc/native/tests/lamb_lars_selftest.cpp (its own
main; the segment / chunk table builder of csrc/kernels/optim_segments.cpp and lamb_step / lars_step of
cpu_ops.cpp against naive per-parameter loops, tiny and ragged slices, an empty parameter, a lone unpadded
parameter and every optional input absent) is compiled with AddressSanitizer + UndefinedBehaviorSanitizer
and run on the CPU (the plain build of the same code is what tests/test_lamb_lars_cpu.py runs). The
sanitizer runtimes are linked statically into the program; nothing sanitized is loaded into Python.
-O0: the compile is the test's cost, the cases are tiny."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dcnn_amd", "csrc", "native")
KSRC = os.path.join(ROOT, "dcnn_amd", "csrc", "kernels")


def test_lamb_lars_selftest_asan_ubsan(tmp_path):
    san = "address,undefined"
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "lamb_lars_selftest")
    flags = ["-O0", "-std=c++17", "-pthread", f"-fsanitize={san}", "-fno-omit-frame-pointer", "-static-libasan",
             "-static-libubsan"]
    cmd = [cxx, *flags, os.path.join(SRC, "tests", "lamb_lars_selftest.cpp"), os.path.join(KSRC, "optim_segments.cpp"),
           os.path.join(SRC, "cpu_ops.cpp"), os.path.join(SRC, "cpu_gemm.cpp"), os.path.join(SRC, "threadpool.cpp"),
           "-I", SRC, "-o", exe, "-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "lamb lars selftest OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
