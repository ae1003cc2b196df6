"""searchsorted / bincount / histogram through the C++ surface on the GPU: tests/cpp/test_count.cpp (member and sm:: forms for the
four element types, what throws std::invalid_argument and std::out_of_range, a view and a pending chain as operands, bincount of an
argmax, the result in an operator chain, the `counts` counter, the README's snippets)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_count_through_the_cpp_surface():
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()["test_count"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
