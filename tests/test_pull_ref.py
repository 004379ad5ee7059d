"""The byte-exact reference of the pull kernels (tests/native/pull_ref.h) and
the comparison that tests/native/pull_kernels_check.hip applies with it: does
it catch a subtly wrong kernel?

The cases live in tests/native/pull_ref_check.cpp, a stand-alone program built
here with AddressSanitizer + UBSan and run as a program (nothing is loaded
into Python).  It holds host emulations of both device walks; unmutated they
match the reference on every table and block count of the GPU harness, and
each of eleven mutations (a stale `first` or `cur`, a wrong tail, a shifted
vector, a skipped tile, a stale granule, a one-sided partition quotient,
exchanged strides, an off-by-one bound) is flagged, with no byte flagged that
a mutated tile does not account for."""
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "pull_ref_check.cpp")

MUTATIONS = ["first_stale", "cur_stale", "nv_roundup", "tail_dropped",
             "tail_shift", "vec_shift", "tile_skipped", "glog_stale",
             "part_src_only", "stride_swap", "bound_le"]
_LINE = re.compile(r"^MUTATION (\w+) +table (\S+) +U (\d+) blocks (\d+) +"
                   r"flagged (\d+) +first (\d+) +\((.*)\) outside (\d+) "
                   r"refused (\d+)$", re.M)


def _compiler():
    # clang first: it links the sanitizer runtime statically, so the program
    # does not care what else the environment loads into every process
    for cxx in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++",
                "clang++", "g++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_pull_ref_sanitized(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path / "pull_ref_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
    assert "unmutated emulation == reference" in run.stdout
    rows = _LINE.findall(run.stdout)
    assert sorted({r[0] for r in rows}) == sorted(MUTATIONS), run.stdout
    for name, table, _u, _g, flagged, _first, where, outside, _ref in rows:
        assert int(flagged) > 0, (name, table)
        assert int(outside) == 0, (name, table)
        assert where, (name, table)
