"""Cumulative scans through the C++ surface on the GPU: tests/cpp/test_scan.cpp (sm:: and member forms for the four element
types, negative and absent axis, a bad axis, a pending chain and a view as operands, the CDF, the `scans` counter, the README's
snippet)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_scans_through_the_cpp_surface():
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()["test_scan"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
