"""What the C ABI's entry points answer to calls they refuse, pinned by a recorded table (tests/golden/abi_errors.json, written by
tests/golden/make_abi_errors.py on a machine without a device): every row is replayed against the built library and the return
code and the FULL message compared for equality -- which check fires first, and its wording, are the contract.  A refusal that
is meant to change is a diff in that table, never an edit here.

Only without a device: the pointers in the table are made-up integers, and a regression that let one of these calls past its
checks would launch on them."""
import json

import pytest

import simplemath_amd as sma
from tests.golden import make_abi_errors as gen

RAW = ("reduce_raw", "scan_raw", "argreduce_raw", "sort_raw", "take_raw", "scatter_raw", "searchsorted_raw", "bincount_raw", "histogram_raw", "unary_raw", "convert_raw",
       "where_raw", "select_count_raw", "select_raw", "runs_count_raw", "runs_raw")
PLANS = ("reduce_plan", "scan_plan", "argreduce_plan", "sort_plan", "take_plan", "scatter_plan", "count_plan", "select_plan", "convert_plan", "runs_plan")


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    lib = sma.load()
    if lib.device_count():
        pytest.skip("a device is present: a call that got past its checks would launch on made-up pointers")
    return lib


@pytest.fixture(scope="module")
def table():
    with open(gen.TABLE) as f:
        return json.load(f)


def test_the_table_holds_exactly_the_generators_cases(table):
    cases = gen.cases()
    assert len(table) == len(cases) and len(table) >= 300
    for row, case in zip(table, cases):
        assert row[:3] == json.loads(json.dumps(case)) and len(row) == 5
        assert row[3] in (gen.OK, gen.INVALID, gen.UNSUPPORTED) and (row[4] == "") == (row[3] == gen.OK)
    assert len({(r[0], r[1], json.dumps(r[2])) for r in table}) == len(table)
    for fn in RAW:
        rows = [r for r in table if r[0] == fn]
        dtypes = {r[2].get("dtype", r[2].get("src_dtype")) for r in rows}
        assert dtypes >= ({sma.I32, sma.I64} if fn == "bincount_raw" else {sma.F32, sma.I64}), fn
        assert sum(r[3] == gen.INVALID for r in rows) >= 10, fn
        # the call with nothing to do; the two counts always have their one word to write
        assert any(r[3] == gen.OK for r in rows) == (fn not in ("select_count_raw", "runs_count_raw")), fn
        assert any("null" in r[1] for r in rows), fn
    for fn in PLANS:
        assert [r[3] for r in table if r[0] == fn and r[1] == "well-formed"] == [gen.OK], fn
        assert any(r[0] == fn and r[3] == gen.INVALID for r in table), fn
    assert {r[0] for r in table} == set(RAW + PLANS)
    assert any(r[3] == gen.UNSUPPORTED for r in table)
    # a null table of non-zero length, with and without a result below that length
    assert {r[3] for r in table if r[0] == "histogram_raw" and "a null table" in r[1]} == {gen.INVALID}


def test_every_row_is_what_the_library_answers(lib, table):
    for fn, name, kwargs, rc, msg in table:
        assert gen.answer(lib, fn, kwargs) == (rc, msg), "%s, %s: %r" % (fn, name, kwargs)
