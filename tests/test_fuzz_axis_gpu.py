"""A short run of tests/fuzz_axis.py on the GPU, in a child process: as it is, and with the grid of every axis family capped at 3
workgroups, so that every loop over tasks runs many times per lane."""
import os
import subprocess
import sys
import time

import pytest

from tests import fuzz_axis
from tests.test_fuzz_axis_host import planned

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPPED = {f"SMHIP_{family}_GRID_CAP": "3" for family in fuzz_axis.GRID_CAPS}
CHILD_TIMEOUT = 180   # seconds; see the docstring below


@pytest.mark.parametrize("env", [{}, CAPPED], ids=["plain", "capped"])
def test_fuzz_axis_smoke(env):
    """SMOKE_CASES cases of seed SMOKE_SEED: exit 0, nothing skipped, and the tables the child prints are, row for row, the ones
    tests/test_fuzz_axis_host.py holds to at least 3 per row.  Measured on an MI355X: 700 cases of at most
    2^20 elements in 6.4 s wall as it is and 6.8 s with the capped grids, the child's start, the first use of every kernel and the
    numpy references included (drawing the cases alone takes 4 s of it on the host).  The child's time limit is 25 times that, for a
    cold start on a busy machine."""
    cases, seed = fuzz_axis.SMOKE_CASES, fuzz_axis.SMOKE_SEED
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_axis.py"), str(cases), str(seed)], capture_output=True, text=True, timeout=CHILD_TIMEOUT,
                       env=dict(os.environ, **env), cwd=ROOT)
    print(f"{time.perf_counter() - t0:.1f} s wall")
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0 and f"ok: {cases} cases" in r.stdout and r.stdout.rstrip().endswith("skipped 0"), tail
    want = fuzz_axis.table_lines(planned())
    got = [line for line in r.stdout.splitlines() if line in want or line.startswith("  ")]
    assert got == want, tail
