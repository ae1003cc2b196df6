"""Functions of one argument, host side: the exp / log evaluations themselves (simplemath_amd/csrc/sm_unary.h, the source the
gfx950 kernels inline) compiled for the CPU and swept, and the C ABI's argument checks -- no device involved."""
import re
import subprocess

import numpy as np
import pytest

import simplemath_amd as sma


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def test_exp_and_log_algorithms_on_host():
    """f32: >= 8 M arguments per function over every binade (subnormals included) plus every value within 64 ULP of exp's
    overflow / underflow thresholds and of 1.0 for log, against glibc's fp64 exp / log of the argument, the error in f32 ULPs of
    that fp64 value.  f64: >= 3.5 M arguments against expl / logl in long double.  Bound: 1 ULP everywhere, nothing excluded;
    the special values bit for bit."""
    from simplemath_amd import build
    exe = build.build_host_programs()["unary_host_check"]
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=600).stdout
    print(out)
    for name, least in (("expf", 8_000_000), ("logf", 8_000_000), ("exp", 3_500_000), ("log", 3_500_000)):
        m = re.search(rf"^{name} max_ulp ([0-9.]+) over (\d+)", out, re.M)
        assert m, out
        assert int(m.group(2)) >= least, out
        assert float(m.group(1)) <= 1.0, out
    assert "lattice_mismatches 0" in out, out


def test_unary_entry_point_is_declared():
    assert "smhip_unary" in sma.declared_symbols()
    assert sma.SMHIP_OP_UNARY_BASE > sma.OP_LEFT and sma.SMHIP_OP_UNARY_BASE + sma.UNARY_LOG < 100  # below SMHIP_OP_USER_BASE


def test_unary_argument_validation_needs_no_gpu(lib):
    f32, i32, i64 = sma.F32, sma.I32, sma.I64
    bad = [
        (5, f32, [1], [4]),               # fn
        (-1, f32, [1], [4]),
        (sma.UNARY_EXP, 9, [1], [4]),     # dtype
        (sma.UNARY_EXP, f32, [1] * 7, [2] * 7),  # ndim > MAX_NDIM
        (sma.UNARY_EXP, f32, [1], [-4]),  # negative extent
        (sma.UNARY_EXP, f32, [-1], [4]),  # negative stride
    ]
    for fn, dtype, strides, shape in bad:
        assert lib.unary_raw(fn, dtype, 4096, strides, shape, 8192) == sma.ERR_INVALID, (fn, dtype, strides, shape)
    assert lib.unary_raw(sma.UNARY_EXP, f32, 4096, None, None, 8192) == sma.ERR_INVALID   # null shape / strides (ndim 0)
    assert lib.unary_raw(sma.UNARY_EXP, f32, 0, [1], [4], 8192) == sma.ERR_INVALID        # null operand
    assert lib.unary_raw(sma.UNARY_EXP, f32, 4096, [1], [4], 0) == sma.ERR_INVALID        # null result
    assert lib.unary_raw(sma.UNARY_EXP, f32, 0, [1], [0], 0) == 0                    # an empty shape is a no-op
    # out overlaps the operand without being it: rejected before anything is launched
    assert lib.unary_raw(sma.UNARY_NEG, f32, 4096, [1], [64], 4096 + 16) == sma.ERR_INVALID
    assert lib.unary_raw(sma.UNARY_NEG, f32, 4096, [2], [64], 4096) == sma.ERR_INVALID    # out == a, but a is a stepped view
    for fn in (sma.UNARY_SQRT, sma.UNARY_EXP, sma.UNARY_LOG):
        for dt in (i32, i64):
            assert lib.unary_raw(fn, dt, 4096, [1], [4], 8192) == sma.ERR_UNSUPPORTED, (fn, dt)
    with pytest.raises(KeyError):
        lib.unary("tanh", None)


def test_unary_chain_stage_validation_needs_no_gpu(lib):
    """smhip_chain's checks of a stage without an operand, through the raw entry point (nothing is launched: every call fails)."""
    import ctypes as C
    U = sma.SMHIP_OP_UNARY_BASE

    def chain(dtype, ptrs, ops, scalars=True):
        n = len(ptrs)
        strides = (C.c_int64 * n)(*([1] * n))
        sc = (C.c_double * n)() if scalars else None
        return lib.c.smhip_chain(C.c_int(dtype), C.c_int(n), (C.c_void_p * n)(*ptrs), strides, sc, (C.c_int * (n - 1))(*ops),
                                 (C.c_int * (n - 1))(*([0] * (n - 1))), (C.c_int64 * 1)(8), C.c_int(1), C.c_void_p(1 << 20))

    assert chain(sma.F32, [4096, 8192], [U + sma.UNARY_EXP]) == sma.ERR_INVALID              # a unary stage with an operand
    assert chain(sma.I32, [4096, None], [U + sma.UNARY_EXP]) == sma.ERR_UNSUPPORTED          # exp of integers
    assert chain(sma.I64, [4096, None], [U + sma.UNARY_SQRT]) == sma.ERR_UNSUPPORTED
    assert chain(sma.F32, [4096, None], [U + 5]) == sma.ERR_UNSUPPORTED                      # no such function
    assert chain(sma.F32, [4096, None], [sma.OP_LEFT]) == sma.ERR_UNSUPPORTED                # (as before)
    assert chain(sma.F32, [4096, None, None], [U + sma.UNARY_NEG, sma.OP_ADD], scalars=False) == sma.ERR_INVALID  # ADD's scalar needs scalars_host
