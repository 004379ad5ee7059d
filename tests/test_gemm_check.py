"""The GEMM checker (bench/gemm_check.h): bf16 conversion, the two input
generators, the float64 reference and the comparison that
`gemm_pready --check` and tests/test_gemm_gpu.py rely on.

The cases live in tests/native/gemm_check_check.cpp, a stand-alone program
built here with AddressSanitizer + UBSan and run as a program (nothing is
loaded into Python).  It shows without a GPU that the GPU test would fail for
a subtly wrong kernel: an emulated kernel passes at every shape of the GPU
test, and each mutation of its output (a dropped k-term, a skipped or doubled
K-tile, exchanged tiles, exchanged tile indices, a transposed sub-block, a
poisoned tile, a truncating conversion) is reported."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "gemm_check_check.cpp")

MUTATIONS = ["drop one k-term", "skip one K-tile", "K-tile twice",
             "two tiles exchanged", "tm/tn exchanged", "sub-block transposed",
             "tile left at poison"]


def _compiler():
    # clang first: it links the sanitizer runtime statically, so the program
    # does not care what else the environment loads into every process
    for cxx in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++",
                "clang++", "g++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_gemm_check_sanitized(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "gemm_check_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
    # every mutation ran, in both data modes
    for name in MUTATIONS:
        for mode in ("unit", "uniform"):
            assert any(line.startswith(name) and f" {mode} " in line
                       for line in run.stdout.splitlines()), (name, mode)
    assert "truncated conversion" in run.stdout
