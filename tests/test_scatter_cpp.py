"""put_along_axis / put / scatter_add / index_add through the C++ surface on the GPU: tests/cpp/test_scatter.cpp (member and sm::
forms for the four element types, negative and absent axis, put_flat, the scalar overloads, what throws std::invalid_argument and
std::out_of_range, a sliced and a transposed target, a pending chain as the values, the result in an operator chain, NaN payloads
and signed zeros, the `scatters` counter, the README's snippets)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_scatter_through_the_cpp_surface():
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()["test_scatter"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
