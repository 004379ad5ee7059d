"""The planner of the strided reducing receive
(src/transport/strided_reduce_plan.h: plan_strided_reduce), its host combine
(src/transport/layout.h: layout_reduce_in) and the reference the GPU harness
compares the strided reduce kernels with (tests/native/strided_reduce_ref.h),
on the CPU: every table of the GPU harness planned, narrow and wide, and
walked on the host the way the kernel walks it, against an element-by-element
reference through part_layout_offset and Red<TYPE>::combine; the unit rule
(16 bytes or one element, never between); tile counts; the batch cut at
overlapping, touching and interleaved extents; what the planner refuses;
layout_reduce_in for chunks that start inside a run; and that the comparison
flags five subtly wrong walks.

The cases live in tests/native/strided_reduce_check.cpp, a stand-alone program
built here with AddressSanitizer + UBSan and run as a program (nothing is
loaded into Python)."""
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "strided_reduce_check.cpp")

MUTATIONS = ["destination gap written",
             "operand dropped in the last partial tile",
             "source and destination offsets swapped",
             "partition quotient ignored",
             "one element combined twice"]


def _compiler():
    # clang first: it links the sanitizer runtime statically, so the program
    # does not care what else the environment loads into every process
    for cxx in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++",
                "clang++", "g++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_strided_reduce_sanitized(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "strided_reduce_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
    for name in MUTATIONS:
        m = re.search(rf"^{name}: (\d+) bytes flagged$", run.stdout, re.M)
        assert m and int(m.group(1)) > 0, name
