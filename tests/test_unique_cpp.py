"""The distinct values through the C++ surface on the GPU: tests/cpp/test_unique.cpp (unique_values / unique / unique_counts /
unique_inverse / unique_all / unique_consecutive / run_lengths, free and member forms, for the four element types and both settings of
equal_nan, views and pending chains as operands, empty operands, take_flat(inverse) rebuilding the operand, unique_counts against
bincount, the group-by through index_add, the `uniques` and `sorts` counters) and the README's snippets (tests/cpp/readme_unique.cpp)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ("test_unique", "readme_unique"))
def test_unique_through_the_cpp_surface(name):
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()[name]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
