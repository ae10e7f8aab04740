"""Exact row intervals of the descriptor window (csrc/sift_desc_rows.h) on the CPU.

tests/cpp/test_desc_rows.cpp includes the header the kernels use and, for more than 20,000 window geometries (random
angles and hist_width 1.5-25, the axis angles and 45 degrees exactly, keypoints within 2 px of every border and
corner, planes down to 6 x 5, every radius 1..63), compares desc_row_interval row by row with the brute-force set of
the oracle's per-sample test over j in [-R-4, R+4]; each job also runs with the reciprocals 2 ulp off, as the
kernels' approximate reciprocal may be.  The kernels' enumerated sample loop has no per-sample test and no bin
clamps: this equality is what keeps its LDS adds inside the histogram.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_row_intervals_equal_brute_force(tmp_path):
    exe = tmp_path / "test_desc_rows"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "another-cuda-sift_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "test_desc_rows.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"ok jobs=(\d+) rows=(\d+) nonempty=(\d+) samples=(\d+) conservative=(\d+) max_trim_lo=(\d+) "
                  r"max_trim_hi=(\d+)", r.stdout)
    assert m, r.stdout
    jobs, rows, nonempty, samples, conservative, trim_lo, trim_hi = map(int, m.groups())
    assert jobs >= 20000 and nonempty > 100 * 1000 and samples > 1000 * 1000
    # the exact intervals lie inside the conservative ones, a few samples in at each end
    assert samples < conservative
    assert trim_lo <= 4 and trim_hi <= 4, (trim_lo, trim_hi)
