"""Choosing by condition through the C++ surface on the GPU: tests/cpp/test_select.cpp (every comparison operator form, sm::where,
assign_where, mask, count_nonzero, flatnonzero, nonzero, select and compress for the four element types, views and pending chains as
operands, empty results, what throws, flatnonzero feeding take_flat and put_flat, the `selects` counter) and the README's snippets
(tests/cpp/readme_select.cpp)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ("test_select", "readme_select"))
def test_select_through_the_cpp_surface(name):
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()[name]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
