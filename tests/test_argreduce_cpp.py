"""argmax / argmin through the C++ surface on the GPU: tests/cpp/test_argreduce.cpp (sm:: and member forms for the four element
types, negative and absent axis, keepdims shapes, a bad axis, a pending chain and a transposed view as operands, max_with_index
against max and argmax called separately, the result in an operator chain, the `arg_reductions` counter, the README's snippets)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_argreduce_through_the_cpp_surface():
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()["test_argreduce"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
