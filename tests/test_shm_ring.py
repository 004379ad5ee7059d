"""The shared-memory descriptor ring (src/transport/shm_ring.h): geometry,
space and stage-credit arithmetic across wrap-arounds, and a producer and a
consumer thread pushing 20 000 descriptors through 4 slots.

The cases live in tests/native/shm_ring_check.cpp, a stand-alone program
built here twice and run as a program (nothing is loaded into Python): with
AddressSanitizer + UBSan, and with ThreadSanitizer, because the ring is the
one lock-free structure two processes share and its memory orders are the
thing under test."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "shm_ring_check.cpp")


def _compiler():
    # clang first: it links the sanitizer runtime statically, so the program
    # does not care what else the environment loads into every process
    for cxx in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++",
                "clang++", "g++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_shm_ring_sanitized(tmp_path, sanitize):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "shm_ring_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
         "-fsanitize=" + sanitize, "-fno-sanitize-recover=undefined",
         "-Wall", "-Wextra", "-Werror", "-pthread", SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
