"""The definition of the reducing receive (src/transport/reduce.h: combine,
reduce_host) and its planner (src/transport/reduce_plan.h: plan_reduce) on
the CPU: all 18 type/op pairs against independent references (float64
rounded once for f16, widen / add / nearest-even for bf16, native types
otherwise) on random values, exact ties of both parities and integer wrap;
merging, the batch cut at an overlapping destination and tile counts of the
plan; and that the comparison flags a truncating bf16 sum and an operand
dropped in the tail.

The cases live in tests/native/reduce_check.cpp, a stand-alone program built
here with AddressSanitizer + UBSan and run as a program (nothing is loaded
into Python)."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "reduce_check.cpp")


def _compiler():
    # clang first: it links the sanitizer runtime statically, so the program
    # does not care what else the environment loads into every process
    for cxx in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++",
                "clang++", "g++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_reduce_sanitized(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "reduce_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
    assert "truncating bf16 sum" in run.stdout
