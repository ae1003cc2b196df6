"""The cases of tests/large_cases.py on the CPU: every shape that test_past_2p31_gpu.py runs plans the route it is meant to reach, is
as large as the case needs, and stages no copy of an operand that is itself large -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma
from tests import large_cases as lc

P31, P32, P33 = lc.P31, lc.P32, lc.P33


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_plan_of_every_case(lib, name):
    case = lc.CASES[name]
    assert lc.plan_of(lib, case) == (case["plan"], case["launches"]), name


def test_the_table_row_by_row(lib):
    """The table of the cases spelt out once more, independent of large_cases.py's own helpers: (route word, launches)."""
    R, M, Y = sma.SORT_ROUTE_ROW, sma.SORT_MERGE, sma.SORT_COPY
    assert lib.sort_plan(np.float32, [2_147_500, 1000], [1000, 1], 1)[:2] == (R, 1)                       # S1
    assert lib.sort_plan(np.int64, [2_147_500, 500], [500, 1], 1)[:2] == (R, 1)                           # S1 as int64
    assert lib.sort_plan(np.float32, [262_129, 8193], [8193, 1], 1)[:2] == (R | M, 3)                     # S2
    assert lib.sort_plan(np.float32, [257, 8_355_984], [8_355_984, 1], 0)[:2] == (R | Y, 4)               # S3
    assert lib.sort_plan(np.float32, [3, 715_829_250], [715_829_250, 1], 0)[:2] == (R | Y, 4)             # S3b
    LINE, ROWS, DIRECT = sma.TAKE_ROUTE_LINE, sma.TAKE_ROUTE_ROWS, sma.TAKE_ROUTE_DIRECT
    rows = (1 << 21) + 5
    assert lib.take_plan(np.float32, [1024, 1], rows, [1, 0], [4096, 1024], 0)[:2] == (ROWS, 1)           # T1
    assert lib.take_plan(np.int64, [512, 1], rows, [1, 0], [4096, 512], 0)[:2] == (ROWS, 1)               # T1 as int64
    assert lib.take_plan(np.float32, [1024, 1], rows, [1024, 1], [8, 1024], 0)[:2] == (DIRECT, 1)         # T2
    assert lib.take_plan(np.float32, [1000, 1], 1000, [0, 1], [2_147_500, 1000], 1)[:2] == (LINE, 1)      # T3
    assert lib.take_plan(np.float32, [1031, 1], 7, [0, 1], [4_165_924, 1031], 0)[:2] == (DIRECT, 1)       # T4
    assert lib.take_plan(np.float32, [1], P31 + 4099, [1], [4096], 0)[:2] == (DIRECT, 1)                  # T5
    D, RW, S, SR = sma.SCATTER_ROUTE_DIRECT, sma.SCATTER_ROUTE_ROWS, sma.SCATTER_ROUTE_SORTED, sma.SCATTER_ROUTE_SORTED_ROWS
    table = [rows, 1024]
    assert lib.scatter_plan(np.float32, table, 0, [1, 0], [1024, 1], 300, unique=True)[:2] == (RW, 1)     # C1
    assert lib.scatter_plan(np.float32, table, 0, [1, 0], [1024, 1], 3000)[:2] == (SR, 3)                 # C2
    assert lib.scatter_plan(np.float32, table, 0, [1024, 1], [1024, 1], 8, unique=True)[:2] == (D, 1)     # C3, unique
    assert lib.scatter_plan(np.float32, table, 0, [1024, 1], [1024, 1], 24)[:2] == (S, 3)                 # C3
    assert lib.scatter_plan(np.float32, [P31 + 4099], 0, [1], [1], 5000)[:2] == (S, 4)                    # C4
    assert lib.scatter_plan(np.float32, [2_147_500, 1000], 1, [0, 1], [0, 1], 1500)[:2] == (S, 3)         # C5
    assert lib.scatter_plan(np.float32, [4_165_924, 1, 1031], 1, [0, 0, 1], [0, 0, 1], 1)[:2] == (D, 1)   # C6
    # PUT or ADD, and the index mode, do not enter a plan
    for kind in (sma.SCATTER_PUT, sma.SCATTER_ADD):
        for mode in ("checked", "clip", "wrap"):
            assert lib.scatter_plan(np.float32, [P31 + 4099], 0, [1], [1], 5000, kind=kind, mode=mode)[:2] == (S, 4)
    for mode in ("checked", "wrap"):
        assert lib.take_plan(np.float32, [1000, 1], 1000, [0, 1], [2_147_500, 1000], 1, mode)[:2] == (LINE, 1)
    assert lib.sort_plan(np.float32, [262_129, 8193], [8193, 1], 1, descending=True)[:2] == (R | M, 3)


def test_the_sizes_the_cases_exist_for():
    c = lc.CASES
    for name, case in c.items():
        assert case["large"] * case["itemsize"] > P32, name              # a byte span above 2^32 in every case
    for name in ("S1", "S2", "S3", "S3b", "T1", "T2", "T3", "T4", "T5", "C1", "C2", "C3", "C3_unique", "C4", "C5", "C6"):
        assert c[name]["large"] > P31, name                              # element 2^31 exists
    for name in ("S1_i64", "T1_i64"):                                   # the same bytes as eight-byte elements: past byte 2^33
        assert c[name]["large"] * 8 > P33, name
    assert c["S1"]["large"] == c["T3"]["large"] == c["C5"]["large"] == P31 + 16_352
    assert c["S1"]["large"] * 8 > 1 << 34                                # S1's int64 positions pass byte 2^34
    assert (c["S1"]["large"] - P31) // lc.LINE == 16                     # 16 whole lines past element 2^31
    assert c["S2"]["large"] == P31 + 139_249
    assert c["S3"]["large"] > P31 and c["S3b"]["large"] > P31
    for name in ("T1", "T2", "C1", "C2", "C3", "C3_unique"):
        assert c[name]["large"] == P31 + 5120, name
    assert (1 << 21) * lc.TABLE_COLS == P31 and (1 << 20) * lc.TABLE_COLS * 4 == P32   # row 2^21 holds element 2^31, row 2^20 starts at byte 2^32
    assert lc.FLAT > P31 and lc.FLAT < P32                               # 2^32 is out of range for T5 / C4
    for name in ("T4", "C6"):                                            # the flat entry counter passes 2^32, the divisor stays small
        assert c[name]["entries"] == P32 + 100_348 and lc.WIDE_COLS < 1 << 16, name
    assert c["C5"]["entries"] == lc.LINES * lc.C5_ENTRIES > P31          # the sorted combine walks more entries than the target has elements
    # a sort axis stays below 2^31 positions (the library refuses more); take and scatter accept FLAT
    for name in ("S1", "S1_i64", "S2", "S3", "S3b"):
        assert c[name]["shape"][c[name]["axis"]] < P31


def test_no_case_copies_a_large_operand(lib):
    """A COPY flag on take or scatter is a dense copy of an operand of the result's size; the sort's staged routes (S3, S3b) are
    the cases for exactly that, and nothing else may carry the flag."""
    for name, case in lc.CASES.items():
        route, _ = lc.plan_of(lib, case)
        flags = route & ~0xff
        if case["family"] == "sort":
            assert bool(flags & sma.SORT_COPY) == (name in ("S3", "S3b")), name
        else:
            assert flags == 0, name
    # the trap: the same picks with a middle axis of 5 plan a dense copy of the broadcast operand, 24 GiB
    trap = lc.T4_TRAP
    assert lc.plan_of(lib, trap)[0] == (sma.TAKE_ROUTE_DIRECT | sma.TAKE_COPY) == trap["plan"]
    assert trap["large"] * 4 > 22 << 30


def test_boundary_lines():
    f = lc.boundary_lines
    # S1: values of 4 bytes and positions of 8
    got = f(lc.LINES, lc.LINE, (4, 8))
    assert got == sorted(set(got)) and all(0 <= x < lc.LINES for x in got)
    first31 = P31 // 1000
    for want in (0, 1, lc.LINES - 2, lc.LINES - 1, first31 - 1, first31, first31 + 1):
        assert want in got
    for size in (4, 8):
        for byte in (P32, P33):
            line = byte // size // 1000
            assert line * 1000 * size <= byte < (line + 1) * 1000 * size
            assert {line - 1, line, line + 1} <= set(got), (size, byte)
    past = [x for x in got if x > first31]
    assert len(past) == 16 and past == list(range(first31 + 1, lc.LINES))   # S1 has exactly 16 lines past element 2^31: all of them
    # many lines past the boundary: 16 of them, evenly, from the first to the last
    got = f(1 << 22, 1024, (4,))
    past = [x for x in got if x > (1 << 21) + 1]
    assert len(past) == 16 and past[0] > (1 << 21) + 1 and past[-1] == (1 << 22) - 1
    steps = np.diff([x for x in past if x < (1 << 22) - 2])
    assert steps.max() - steps.min() <= 1
    assert {(1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 21) - 1, 1 << 21, (1 << 21) + 1} <= set(got)
    # an array that ends before a boundary leaves it out; a tiny one is just its lines
    got = f(lc.LINES, 500, (8,))                       # S1 as int64: 2^30 + ... elements, so no element 2^31
    assert max(got) == lc.LINES - 1 and P33 // 8 // 500 in got and P32 // 8 // 500 in got and P31 // 500 >= lc.LINES
    assert f(3, 10, (4,)) == [0, 1, 2] and f(1, 10, (4, 8)) == [0]
    # the cases' own samples stay small: a test downloads a few dozen lines
    for lines, R, sizes in ((lc.LINES, lc.LINE, (4, 8)), (lc.S2_LINES, lc.S2_LINE, (4,)), (lc.S3_COLS, lc.S3_ROWS, (4,)), (lc.S3B_COLS, lc.S3B_ROWS, (4,))):
        assert 20 <= len(f(lines, R, sizes)) <= 48
