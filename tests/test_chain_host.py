"""smhip_chain's rule for a result that shares memory with an operand (include/smhip.h), through the raw entry point with
made-up addresses: `out` may BE an operand that is dense over the result's shape (in place); every other overlap is
SMHIP_ERR_INVALID before a device is touched.  No device involved: every call here fails one way or the other."""
import ctypes as C

import pytest

import simplemath_amd as sma


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


ROWS, COLS = 6, 8
DENSE, STEPPED, ROW, COLUMN, TRANSPOSED = (COLS, 1), (2 * COLS, 2), (0, 1), (1, 0), (1, ROWS)


def _chain(lib, dtype, operands, ops, out, shape=(ROWS, COLS)):
    """operands: (address or None, strides in elements) per operand -> smhip_chain's return code"""
    n, nd = len(operands), len(shape)
    ptrs = (C.c_void_p * n)(*[p for p, _ in operands])
    strides = (C.c_int64 * (n * nd))(*[s for _, st in operands for s in st])
    scalars = (C.c_double * n)()
    return lib.c.smhip_chain(C.c_int(dtype), C.c_int(n), ptrs, strides, scalars, (C.c_int * (n - 1))(*ops),
                             (C.c_int * (n - 1))(*([0] * (n - 1))), (C.c_int64 * nd)(*shape), C.c_int(nd), C.c_void_p(out))


@pytest.mark.parametrize("dtype,esz", [(sma.F32, 4), (sma.F64, 8), (sma.I64, 8)], ids=["f32", "f64", "i64"])
def test_chain_rejects_a_result_that_overlaps_an_operand(lib, dtype, esz):
    A, B, FAR = 1 << 20, 1 << 21, 1 << 22
    n = ROWS * COLS
    add = [sma.OP_ADD]
    # shifted by one element into the head / into a later operand, from either side
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], add, A + esz) == sma.ERR_INVALID
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], add, A - esz) == sma.ERR_INVALID
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], add, B + esz) == sma.ERR_INVALID
    assert _chain(lib, dtype, [(A, DENSE), (None, (0, 0)), (B, DENSE)], [sma.OP_MUL, sma.OP_ADD], B - esz) == sma.ERR_INVALID
    assert "overlaps operand 2" in lib.c.smhip_last_error().decode()
    # one shared byte: out begins on the operand's last byte / ends on its first
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], add, A + n * esz - 1) == sma.ERR_INVALID
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], add, B - n * esz + 1) == sma.ERR_INVALID
    # out == an operand that is not dense over the result's shape
    assert _chain(lib, dtype, [(A, STEPPED), (B, DENSE)], add, A) == sma.ERR_INVALID
    assert _chain(lib, dtype, [(A, DENSE), (B, ROW)], add, B) == sma.ERR_INVALID
    assert _chain(lib, dtype, [(A, DENSE), (B, COLUMN)], add, B) == sma.ERR_INVALID
    assert _chain(lib, dtype, [(A, DENSE), (B, TRANSPOSED)], add, B) == sma.ERR_INVALID
    # a row that ends before out begins shares nothing with it -- the probe below tells "passed the overlap rule" from "rejected by it":
    # a stage that is no chain operator is reported (UNSUPPORTED) only after the overlap rule has let the call through
    bad = [sma.OP_LEFT]
    assert _chain(lib, dtype, [(A, DENSE), (B, ROW)], bad, B + COLS * esz) == sma.ERR_UNSUPPORTED
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], bad, FAR) == sma.ERR_UNSUPPORTED
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], bad, A + esz) == sma.ERR_INVALID       # (the probe does not mask a rejection)
    # in place: out == a dense operand -- the head, a later operand, several operands at once; an extent of 1 takes any stride
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], bad, A) == sma.ERR_UNSUPPORTED
    assert _chain(lib, dtype, [(A, DENSE), (B, DENSE)], bad, B) == sma.ERR_UNSUPPORTED
    assert _chain(lib, dtype, [(A, DENSE), (A, DENSE), (B, ROW)], [sma.OP_MUL, sma.OP_LEFT], A) == sma.ERR_UNSUPPORTED
    assert _chain(lib, dtype, [(A, (0, 1)), (B, (7, 1))], bad, A, shape=(1, COLS)) == sma.ERR_UNSUPPORTED
    # ... but not when another operand overlaps it as well
    assert _chain(lib, dtype, [(A, DENSE), (A + esz, DENSE)], bad, A) == sma.ERR_INVALID
    # an empty result overlaps nothing
    assert _chain(lib, dtype, [(A, (1, 1)), (B, (1, 1))], add, A + esz, shape=(0, COLS)) == 0
