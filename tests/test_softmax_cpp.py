"""softmax, log_softmax and logsumexp through the C++ surface on the GPU: tests/cpp/test_softmax.cpp (the free and the member forms
for float and double against a long double evaluation with the header's bounds, negative and absent axis, keepdims, a transposed
view, a sliced view and a pending chain as operands, the result feeding argmax, take_along_axis and an operator chain, the
`softmaxes` counter, what throws std::runtime_error, special lines) and tests/cpp/readme_softmax.cpp (the README's snippet)."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("program", ("test_softmax", "readme_softmax"))
def test_softmax_through_the_cpp_surface(program):
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()[program]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
