"""
The row -> strip rule of the lattice-row strips (deconv3d_amd/csrc/d3d_strips.h, host-only) without
a device: tests/strips_check.cpp, a stand-alone program with its own main, is compiled with the host
compiler and -fsanitize=address,undefined and run as a child process.  Over H in {11 .. 40, 300},
fh in {3, 5, 11}, every cy and S in {2, 3, 4} it asserts that every lattice row, virtual ones
included, is in exactly one strip, that strips are contiguous, that the cube-row bands of different
strips are disjoint for every cy, and that a strip count that leaves a strip with fewer than two
lattice rows is refused.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deconv3d_amd", "csrc")


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no host C++ compiler (c++, g++, clang++) on PATH")


def test_row_to_strip_rule(tmp_path):
    exe = str(tmp_path / "strips_check")
    build = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                            os.path.join(ROOT, "tests", "strips_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout
    words = run.stdout.split()
    assert words[0] == "ok", run.stdout
    plans, refused = int(words[1]), int(words[2])
    # 3 FSF heights x 3 strip counts x 31 cube heights, each planned or refused; both happen
    assert plans + refused == 3 * 3 * 31 and plans > 0 and refused > 0, run.stdout
