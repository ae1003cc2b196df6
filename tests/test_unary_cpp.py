"""Functions of one argument through the C++ surface and over every float on the GPU: tests/cpp/test_unary.cpp (sm::exp / log /
sqrt / abs and unary minus on lvalues, temporaries and views; the README's softmax, log-sum-exp and standard deviation; the
fusion counters) and tests/cpp/unary_exhaustive.hip (all 2^32 bit patterns through smhip_unary)."""
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def _exe(name):
    from simplemath_amd import build
    build.build_lib()
    return build.build_host_programs()[name]


def test_unary_functions_through_the_cpp_surface():
    r = subprocess.run([_exe("test_unary")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("fn", ["exp", "log", "sqrt"])
def test_exhaustive_over_every_float(fn):
    """All 2^32 bit patterns against the fp64 device libm value rounded to f32: nothing beyond 1 ULP (sqrt: nothing beyond 0),
    and the largest distance from the fp64 value itself, in f32 ULPs, at most 1 (sqrt: one half).
    The correctly rounded share is on record in profiles/unary_accuracy.txt."""
    r = subprocess.run([_exe("unary_exhaustive"), fn], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    m = re.search(r"over all (\d+) float bit patterns: 0 ULP (\d+) \(([\d.]+) %\)  1 ULP (\d+) \([\d.]+ %\)  2 ULP (\d+)  >2 ULP (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) == 1 << 32, r.stdout
    assert int(m.group(5)) == 0 and int(m.group(6)) == 0, r.stdout
    if fn == "sqrt":
        assert int(m.group(4)) == 0, r.stdout
    e = re.search(r"largest error against the fp64 value: ([\d.]+) ULP", r.stdout)
    assert e and float(e.group(1)) <= (0.5 if fn == "sqrt" else 1.0), r.stdout
    assert r.returncode == 0, r.stdout + r.stderr
