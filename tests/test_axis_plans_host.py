"""The planners of the axis reductions, the scans and argmax / argmin, pinned by a recorded table (tests/golden/axis_plans.json,
written by tests/golden/make_axis_plans.py): every row is replayed against the built library, field by field -- no device
involved.  A change to a planner heuristic is a diff in that table, never an edit here."""
import json

import pytest

import simplemath_amd as sma
from tests.golden import make_axis_plans as gen


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


@pytest.fixture(scope="module")
def table():
    with open(gen.TABLE) as f:
        return json.load(f)


FIELDS = ("family", "kind", "dtype", "shape", "strides", "axis", "route word", "launches", "(O, R, I)", "chunk")


def test_the_table_holds_exactly_the_generators_cases(table):
    cases = gen.cases()
    assert len(table) == len(cases) and len(table) >= 2000
    for row, case in zip(table, cases):
        assert tuple(row[:6]) == case
        assert len(row) == (9 if row[0] == "reduce" else 10)
    for nd in (1, 2, 3, 4):
        for dt in gen.DTYPES:
            for fam in gen.KINDS:
                assert any(r[0] == fam and r[2] == dt and len(r[3]) == nd for r in table), (nd, dt, fam)
    assert {e for r in table for e in r[3]} >= set(gen.EXTENTS)


def test_every_row_is_what_the_planner_answers(lib, table):
    for row in table:
        got = gen.answer(lib, tuple(row[:6]))
        for name, want, have in zip(FIELDS, row, got):
            assert have == want, "%s: %s is %r, recorded %r" % (row[:6], name, have, want)


# ---- the branches: a row is (family, kind, dtype, shape, strides, axis, route word, launches, [O, R, I], chunk)
def _loads(r):  # 16-byte vectors, then the tail elements one per lane
    W, R = 4 if r[2] == "f32" else 2, r[8][1]
    return R // W + R % W


def _route(r):
    return r[6] & 0xff


def _flag(r, f):
    return bool(r[6] & f)


def _zero_stride(r):
    return any(e > 1 and s == 0 for e, s in zip(r[3], r[4]))


def _permuted(r):  # strides that are the dense ones in another order
    return r[4] != gen.dense(r[3]) and sorted(r[4]) == sorted(gen.dense(r[3]))


def _groups(r):  # runs of reduced axes in index order, size-1 axes dropped
    red = [d in r[5] for d, e in enumerate(r[3]) if e > 1]
    return sum(1 for k, x in enumerate(red) if x and (k == 0 or not red[k - 1]))


def _chunks(r):
    return -(-r[8][1] // r[9])


def _short(route, lo, hi):
    return lambda r: _route(r) == route and r[8][1] > 1 and lo < _loads(r) <= hi and not _flag(r, 0x100)


def _scan_row(O=None, R=None, split=None, dt="f32"):
    return lambda r: (_route(r) == sma.SCAN_ROUTE_ROW and r[2] == dt and _loads(r) > 64 and (O is None or r[8][0] == O) and (R is None or r[8][1] == R)
                      and (split is None or _flag(r, sma.SCAN_SPLIT) == split))


def _scan_col(groups=None, R=None, split=None, dt="f32"):
    return lambda r: (_route(r) == sma.SCAN_ROUTE_COLUMN and r[2] == dt and (groups is None or r[8][0] * -(-r[8][2] // 64) == groups)
                      and (R is None or r[8][1] == R) and (split is None or _flag(r, sma.SCAN_SPLIT) == split))


S, Y, P = sma.ROUTE_SPLIT, sma.ROUTE_COPY, sma.ROUTE_PASSES
BRANCHES = {
    "reduce": {
        "short rows, g = 4": _short(sma.ROUTE_ROW, 0, 4),
        "short rows, g = 16": _short(sma.ROUTE_ROW, 4, 16),
        "short rows, g = 64": _short(sma.ROUTE_ROW, 16, 64),
        "short rows, g = 64, f64": lambda r: _short(sma.ROUTE_ROW, 16, 64)(r) and r[2] == "f64",
        "long rows": lambda r: r[6] == sma.ROUTE_ROW and _loads(r) > 64 and r[7] == 1,
        "long rows, split": lambda r: r[6] == sma.ROUTE_ROW | S and r[7] == 2,
        "columns": lambda r: r[6] == sma.ROUTE_COLUMN and r[7] == 1,
        "columns, split": lambda r: r[6] == sma.ROUTE_COLUMN | S and r[7] == 2,
        "channel": lambda r: r[6] == sma.ROUTE_CHANNEL and r[7] == 1 and r[8][2] <= 8 and r[8][1] >= 1024,
        "channel, split": lambda r: r[6] == sma.ROUTE_CHANNEL | S and r[7] == 2,
        "fill": lambda r: r[6] == sma.ROUTE_FILL and r[7] == 1 and r[8][1] == 0,
        "gather": lambda r: r[6] == sma.ROUTE_GATHER and r[7] == 1,
        "none": lambda r: r[6] == sma.ROUTE_NONE and r[7] == 0,
        "two reduced groups": lambda r: _flag(r, P) and not _flag(r, Y) and _groups(r) == 2 and r[7] >= 2,
        "two reduced groups, a pass split": lambda r: _flag(r, P) and _flag(r, S) and _groups(r) == 2 and r[7] >= 3,
        "three reduced groups": lambda r: _flag(r, P) and _groups(r) == 3 and r[7] >= 3,
        "a copy because of a stride 0": lambda r: _flag(r, Y) and _zero_stride(r),
        "a copy because kept axes do not merge": lambda r: _flag(r, Y) and not _flag(r, P) and _permuted(r) and _groups(r) == 1,
        "a copy of a stepped view": lambda r: _flag(r, Y) and not _zero_stride(r) and not _permuted(r),
        "a transposed view read in place": lambda r: not _flag(r, Y) and _permuted(r) and _route(r) in (sma.ROUTE_ROW, sma.ROUTE_COLUMN) and len(r[3]) == 2 and min(r[3]) > 1,
    },
    "scan": {
        "copy only": lambda r: r[6] == sma.SCAN_ROUTE_COPYONLY and r[7] == 1 and r[8][1] == 1,
        "none": lambda r: r[6] == sma.SCAN_ROUTE_NONE and r[7] == 0,
        "short rows, g = 4": _short(sma.SCAN_ROUTE_ROW, 0, 4),
        "short rows, g = 16": _short(sma.SCAN_ROUTE_ROW, 4, 16),
        "short rows, g = 64": _short(sma.SCAN_ROUTE_ROW, 16, 64),
        "long rows": lambda r: r[6] == sma.SCAN_ROUTE_ROW and _loads(r) > 64 and r[7] == 1 and r[9] == r[8][1],
        "long rows, split": lambda r: r[6] == sma.SCAN_ROUTE_ROW | sma.SCAN_SPLIT and r[7] == 2 and 1 < _chunks(r),
        "rows: 1023 of them are split": _scan_row(O=1023, split=True),
        "rows: 1024 of them are not": _scan_row(O=1024, R=1 << 16, split=False),
        "rows: nor 1025": _scan_row(O=1025, R=1 << 16, split=False),
        "rows: less than two tiles are not split": _scan_row(O=4, R=8191, split=False),
        "rows: two tiles are": lambda r: _scan_row(O=4, R=8192, split=True)(r) and r[9] == 4096,
        "rows: and a little more": lambda r: _scan_row(O=4, R=8193, split=True)(r) and r[9] == 8192,
        "rows, f64: less than two tiles": _scan_row(O=4, R=4095, split=False, dt="f64"),
        "rows, f64: two tiles": lambda r: _scan_row(O=4, R=4096, split=True, dt="f64")(r) and r[9] == 2048,
        "rows: at most 256 chunks": lambda r: _scan_row(O=1, split=True)(r) and r[8][1] >= 1024 * 4096 and _chunks(r) == 256,
        "columns": lambda r: r[6] == sma.SCAN_ROUTE_COLUMN and r[7] == 1 and r[9] == r[8][1],
        "columns, split": lambda r: r[6] == sma.SCAN_ROUTE_COLUMN | sma.SCAN_SPLIT and r[7] == 2 and 1 < _chunks(r),
        "columns: 63 workgroups are split": _scan_col(groups=63, R=4096, split=True),
        "columns: 64 are not": _scan_col(groups=64, R=4096, split=False),
        "columns: nor 65": _scan_col(groups=65, R=4096, split=False),
        "columns: less than two blocks are not split": _scan_col(groups=1, R=511, split=False),
        "columns: two blocks are": lambda r: _scan_col(groups=1, R=512, split=True)(r) and r[9] == 256,
        "columns: and a little more": lambda r: _scan_col(groups=1, R=513, split=True)(r) and r[9] == 512,
        "columns, f64: less than two blocks": _scan_col(groups=1, R=255, split=False, dt="f64"),
        "columns, f64: two blocks": lambda r: _scan_col(groups=1, R=256, split=True, dt="f64")(r) and r[9] == 128,
        "columns: at most 1024 chunks": lambda r: _scan_col(groups=1, split=True)(r) and r[8][1] >= 2048 * 256 and _chunks(r) == 1024,
        "a copy of a transposed view": lambda r: _flag(r, sma.SCAN_COPY) and _permuted(r),
        "a copy because of a stride 0": lambda r: _flag(r, sma.SCAN_COPY) and _zero_stride(r),
        "a copy of a sub-block": lambda r: _flag(r, sma.SCAN_COPY) and len(r[3]) == 2 and r[4][1] == 1 and r[4][0] > r[3][1] > 1,
        "a copy and a split": lambda r: r[6] & 0xf00 == sma.SCAN_COPY | sma.SCAN_SPLIT and r[7] == 3,
    },
    "argreduce": {
        "none": lambda r: r[6] == sma.ARG_ROUTE_NONE and r[7] == 0,
        "short rows, g = 4": _short(sma.ARG_ROUTE_ROW, 0, 4),
        "short rows, g = 16": _short(sma.ARG_ROUTE_ROW, 4, 16),
        "short rows, g = 64": _short(sma.ARG_ROUTE_ROW, 16, 64),
        "long rows": lambda r: r[6] == sma.ARG_ROUTE_ROW and _loads(r) > 64 and r[7] == 1 and r[9] == r[8][1],
        "long rows, split": lambda r: r[6] == sma.ARG_ROUTE_ROW | sma.ARG_SPLIT and r[7] == 2 and 1 < _chunks(r) <= 4096,
        "columns": lambda r: r[6] == sma.ARG_ROUTE_COLUMN and r[7] == 1 and r[9] == r[8][1] > 1,
        "columns, split": lambda r: r[6] == sma.ARG_ROUTE_COLUMN | sma.ARG_SPLIT and r[7] == 2 and 1 < _chunks(r) <= 4096,
        "more than 4096 chunks: two finishing launches": lambda r: r[6] & 0xf00 == sma.ARG_SPLIT and r[7] == 3 and _chunks(r) > 4096,
        "... of f64 as well": lambda r: r[6] & 0xf00 == sma.ARG_SPLIT and r[7] == 3 and _chunks(r) > 4096 and r[2] == "f64",
        "rows: a chunk clamped by 2^31": lambda r: _route(r) == sma.ARG_ROUTE_ROW and r[8][1] >= 1 << 33 and r[9] == 1 << 31 and r[8][0] * 64 >= 1 << 18,
        "columns: a chunk clamped by 2^31": lambda r: (_route(r) == sma.ARG_ROUTE_COLUMN and r[8][1] >= 1 << 33 and r[9] <= 1 << 31 and _flag(r, sma.ARG_SPLIT)
                                                      and r[8][0] * -(-r[8][2] // 4) >= 1 << 18),
        "R = 1, columns": lambda r: r[6] == sma.ARG_ROUTE_COLUMN and r[8][1] == 1 and r[9] == 1 and r[7] == 1,
        "R = 1, rows": lambda r: r[6] == sma.ARG_ROUTE_ROW and r[8][1] == 1 and r[9] == 1 and r[7] == 1,
        "R = 1, a copy": lambda r: _flag(r, sma.ARG_COPY) and r[8][1] == 1 and r[7] == 2,
        "a copy because of a stride 0": lambda r: _flag(r, sma.ARG_COPY) and _zero_stride(r),
        "a copy because kept axes do not merge": lambda r: _flag(r, sma.ARG_COPY) and _permuted(r),
        "a copy of a stepped view": lambda r: _flag(r, sma.ARG_COPY) and not _zero_stride(r) and not _permuted(r),
        "a copy and a split": lambda r: r[6] & 0xf00 == sma.ARG_COPY | sma.ARG_SPLIT and r[7] == 3,
        "a transposed view read in place": lambda r: not _flag(r, sma.ARG_COPY) and _permuted(r) and len(r[3]) == 2 and min(r[3]) > 1,
        "a sub-block read in place": lambda r: not _flag(r, sma.ARG_COPY) and len(r[3]) == 2 and r[4][1] == 1 and r[4][0] > r[3][1] > 1,
    },
}


@pytest.mark.parametrize("family", sorted(BRANCHES))
def test_the_table_reaches_every_branch(table, family):
    rows = [r for r in table if r[0] == family]
    missing = [name for name, reaches in BRANCHES[family].items() if not any(reaches(r) for r in rows)]
    assert not missing, "%s: no row of the table reaches %s" % (family, missing)
