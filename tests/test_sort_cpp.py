"""sort / argsort through the C++ surface on the GPU: tests/cpp/test_sort.cpp (sm:: and member forms for the four element types,
negative and absent axis, the _flat forms, sort_with_index, a bad axis, a transposed view and a pending chain as operands, the
sorted result in an operator chain and a slice, NaN and signed zeros, the `sorts` counter, the README's snippets)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_sort_through_the_cpp_surface():
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()["test_sort"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
