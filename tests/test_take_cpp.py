"""take / take_along_axis through the C++ surface on the GPU: tests/cpp/test_take.cpp (sm:: and member forms for the four element
types, negative and absent axis, take_flat, what throws std::invalid_argument and std::out_of_range, the three index modes, a
transposed view, a slice of an argsort result and a pending chain as operands, the result in an operator chain, NaN payloads and
signed zeros, the `takes` counter, the README's snippets)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_take_through_the_cpp_surface():
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()["test_take"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
