"""
The chained order of the lattice-row strips (deconv3d_amd/csrc/d3d_strip_order.h, host-only: the
schedule d3d_sweep.hip executes) without a device: tests/strip_order_check.cpp, a stand-alone program
with its own main, is compiled with the host compiler, -fsanitize=address,undefined and -Werror and run
as a child process.  Over H in {11 .. 40, 300}, fh in {3, 5, 11}, S in {2, 3, 4}, M in {1, 2, 3}, with
and without the smoothness prior, with every colour active, one whole colour row inactive and single
colours inactive, it lists every launch of three consecutive sweeps with what it reads and writes
(cube rows, G buffer slot rows, spaxel rows), computes happens-before from stream order plus the
schedule's events, and asserts that every conflicting pair is ordered in the sequential colour
order.  The same schedule without its DOWN waits, without its UP waits and without its sweep-end join
must each report a conflict.
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


def test_chained_schedule_orders_every_conflict(tmp_path):
    exe = str(tmp_path / "strip_order_check")
    build = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                            os.path.join(ROOT, "tests", "strip_order_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout
    words = run.stdout.split()
    assert words[0] == "ok", run.stdout
    proved, refused_plan, refused_short, controls = (int(w) for w in words[1:5])
    # (31 cube heights with fw = 4, the flagship height also with square taps) x 3 FSF heights x 3 strip
    # counts, each planned or refused by the strips' plan; a planned one x 3 layer counts x 3 colour sets,
    # each proved or refused for a colour row of fewer than M colours; three controls per full colour set
    plans = (31 + 1) * 3 * 3 - refused_plan
    assert refused_plan > 0 and plans > 0, run.stdout
    assert proved + refused_short == plans * 3 * 3 and refused_short > 0, run.stdout
    assert controls == plans * 3 * 3, run.stdout
