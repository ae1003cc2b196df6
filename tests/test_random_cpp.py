"""sm::Generator through the C++ surface: tests/cpp/test_random.cpp (every method against the definition written out on the host, the
advance of offset() and seek() reproducing a draw, the dropout line as one chain launch after the mask, the in-place forms, a target
that is not dense throwing) and tests/cpp/readme_random.cpp (the README's snippet)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def _exe(name):
    from simplemath_amd import build
    build.build_lib()
    return build.build_host_programs()[name]


def test_generator_through_the_cpp_surface():
    r = subprocess.run([_exe("test_random")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_readme_snippet_compiles_and_runs():
    r = subprocess.run([_exe("readme_random")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "readme_random: 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
