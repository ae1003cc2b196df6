"""astype through the C++ surface: tests/cpp/test_astype.cpp (a.astype<U>() / sm::astype<U>(a) for every pair of the four element types on
named arrays, chain temporaries, transposed views and slices; the result as an operand of the next chain, of take and of cumsum) and
tests/cpp/readme_astype.cpp (the README's examples with data whose answers are known)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def _exe(name):
    from simplemath_amd import build
    build.build_lib()
    return build.build_host_programs()[name]


def test_astype_through_the_cpp_surface():
    r = subprocess.run([_exe("test_astype")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_readme_examples_compile_and_run():
    r = subprocess.run([_exe("readme_astype")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "readme_astype: 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
