"""Runs of strided or gapped partitions, the pure logic: part_layout_offset
and part_layout_fold (src/transport/layout.h), the partition level of the
strided plan (strided_plan.h) and the run decisions that now follow the
request's part stride (part_run.h).

The cases live in tests/native/part_layout_check.cpp, a stand-alone program
built here with AddressSanitizer + UBSan and run as a program (nothing is
loaded into Python)."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "part_layout_check.cpp")


def _compiler():
    # clang first: it links the sanitizer runtime statically, so the program
    # does not care what else the environment loads into every process
    for cxx in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++",
                "clang++", "g++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_part_layout_sanitized(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "part_layout_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
