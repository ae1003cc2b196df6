"""Axis reductions through the C++ surface on the GPU: tests/cpp/test_axis_reduce.cpp (sm:: and member forms, negative and
listed axes, a pending chain and a recorded tiny operator as operands, the normalisation as reductions plus one chain)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_axis_reductions_through_the_cpp_surface():
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()["test_axis_reduce"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
