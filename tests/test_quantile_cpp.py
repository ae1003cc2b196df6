"""quantile, percentile and median through the C++ surface: tests/cpp/test_quantile.cpp (sm::quantile with one probability and a
list, sm::percentile, sm::median, the member forms and the forms without an axis for float and double against the contract applied to
sorted lines on the host, negative axes, keepdims, views and a pending chain as operands, the results fed into an operator chain,
what throws std::invalid_argument, NaN, zeros and infinities, the `quantiles` counter) and tests/cpp/readme_quantile.cpp (the README's
snippet) on the GPU; and, without one, the static_assert that refuses integer arrays at compile time."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CXX = os.environ.get("CXX", "g++")


@pytest.mark.gpu
@pytest.mark.parametrize("program", ("test_quantile", "readme_quantile"))
def test_quantile_through_the_cpp_surface(program):
    from simplemath_amd import build
    build.build_lib()
    exe = build.build_host_programs()[program]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("call", ("sm::median(a, 0)", "a.quantile(0.5, -1)", "sm::percentile(a, {25.0, 75.0}, 0)", "a.median()"))
@pytest.mark.parametrize("element", ("int", "std::int64_t"))
def test_integer_arrays_are_a_compile_error_that_says_what_to_do(element, call):
    prog = f"#include <sm.h>\n#include <cstdint>\nint main() {{ sm::SMArray<{element}> a = sm::ones<{element}>(3, 4); auto r = {call}; (void)r; }}\n"
    r = subprocess.run([CXX, "-std=c++20", "-fsyntax-only", f"-I{INC}", "-x", "c++", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode != 0 and "static assertion failed" in r.stderr
    assert "quantile / percentile / median: float and double only (astype first)" in r.stderr


def test_the_same_calls_compile_for_float_and_double():
    prog = ("#include <sm.h>\nint main() { auto a = sm::ones<float>(3, 4); auto b = sm::ones<double>(3, 4);\n"
            "auto r = sm::median(a, 0); auto s = b.quantile(0.5, -1); auto t = sm::percentile(a, {25.0, 75.0}, 0); auto u = b.median(); (void)r; (void)s; (void)t; (void)u; }\n")
    r = subprocess.run([CXX, "-std=c++20", "-fsyntax-only", f"-I{INC}", "-x", "c++", "-"], input=prog, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
