"""tests/cpp/fuzz_surface.cpp on the GPU: random programs over a pool of named sm::SMArray<T>, through include/sm.h and on the host
model, every observation compared (arrays bit for bit).  Two seeds with the tiny-operator recorder on, the first one again with
SMHIP_TINY_BATCH=0 in a fresh child: the same bytes must come out.  The coverage the runs reach is settled without a device by
tests/test_fuzz_surface_host.py; the runs only have to print the same table."""
import functools
import os
import re
import subprocess
import time

import pytest

from tests.test_fuzz_surface_host import CASES, SEEDS, planned, table_lines

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 240   # seconds; a run takes 1.2 - 1.4 s wall on an MI355X (96 cases, 260 - 300 MB compared): the rest is for a cold start on a busy machine


def _exe():
    from simplemath_amd import build
    build.build_lib()
    return build.build_host_programs()["fuzz_surface"]


@functools.lru_cache(maxsize=None)
def ran(seed, batched):
    """One run of CASES cases of `seed` in a child process: (stdout, what its last lines report)."""
    env = dict(os.environ)
    env.pop("SMHIP_TINY_BATCH", None)
    if not batched:
        env["SMHIP_TINY_BATCH"] = "0"
    t0 = time.perf_counter()
    r = subprocess.run([_exe(), "--seed", str(seed), "--cases", str(CASES)], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
    print(f"seed {seed} batched {batched}: {time.perf_counter() - t0:.1f} s wall")
    tail = r.stdout[-8000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    report = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(fusion|tiny|queues|hash): (.*)$", line)
        if m and m.group(1) == "hash":
            report["hash"] = m.group(2).split()[0]
        elif m:
            report.update({f"{m.group(1)}.{k}": int(v) for k, v in re.findall(r"([a-z_]+) (\d+)", m.group(2))})
    m = re.search(r"^fuzz_surface seed (\d+): (\d+) cases, (\d+) mismatches$", r.stdout, re.M)
    assert m, tail
    report["cases"], report["mismatches"] = int(m.group(2)), int(m.group(3))
    return r.stdout, report


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_surface_with_the_tiny_batch(seed):
    """CASES cases of each seed: no mismatch, the table the host test holds to 5 per row, and every mechanism reached: chains, direct
    assignments, summed chains, operators that stayed alone, recorded tiny operators and operators that took the other queue."""
    stdout, report = ran(seed, True)
    assert report["cases"] == CASES and report["mismatches"] == 0, stdout[-8000:]
    assert table_lines(stdout) == planned(seed)[2], stdout[-8000:]
    for counter in ("fusion.chains", "fusion.direct_assignments", "fusion.summed_chains", "fusion.single_ops", "tiny.operators", "queues.alternations"):
        assert report[counter] > 0, (counter, report)


def test_fuzz_surface_without_the_tiny_batch():
    """The first seed again with SMHIP_TINY_BATCH=0: nothing is recorded, and the hash over every compared device byte is the same."""
    stdout, report = ran(SEEDS[0], False)
    assert report["cases"] == CASES and report["mismatches"] == 0, stdout[-8000:]
    assert report["tiny.operators"] == 0 and report["tiny.launches"] == 0, report
    assert report["hash"] == ran(SEEDS[0], True)[1]["hash"], (report, ran(SEEDS[0], True)[1])
