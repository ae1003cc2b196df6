"""tests/fuzz_axis.py without a device: the cases the GPU smoke runs (its count, its seed) are drawn and the host planners asked.
The soak's coverage is decided here, on the CPU: every row of its tables is reached at least 3 times by the generator alone, so the
GPU smoke (tests/test_fuzz_axis_gpu.py) cannot fail for a coverage reason -- it only has to print the same tables."""
import functools

import pytest

import simplemath_amd as sma
from tests import fuzz_axis


@pytest.fixture(scope="module", autouse=True)
def built():
    from simplemath_amd import build
    build.build_lib()


@functools.lru_cache(maxsize=None)
def planned():
    """The coverage counts of the smoke's cases (fuzz_axis.run without a device); a planner that refuses a case raises here."""
    stats = fuzz_axis.run(sma.load(), fuzz_axis.SMOKE_CASES, fuzz_axis.SMOKE_SEED, plan_only=True)
    assert stats is not None
    return stats


def test_no_case_is_skipped_or_refused():
    stats = planned()
    assert stats["done"] == fuzz_axis.SMOKE_CASES
    assert sum(stats["rows"].values()) + fuzz_axis.SMOKE_CASES // 5 == fuzz_axis.SMOKE_CASES   # every fifth case is a pipeline


def test_every_planner_row_is_reached():
    stats = planned()
    assert sorted(stats["rows"]) == sorted((f, r) for f in fuzz_axis.FAMILIES for r in fuzz_axis.ROWS[f])
    thin = {k: n for k, n in stats["rows"].items() if n < 3}
    assert not thin, thin


def test_every_view_trait_is_reached_in_every_family():
    stats = planned()
    assert len(stats["traits"]) == len(fuzz_axis.TRAITS) * len(fuzz_axis.FAMILIES)
    thin = {k: n for k, n in stats["traits"].items() if n < 3}
    assert not thin, thin


def test_every_pipeline_row_is_reached():
    stats = planned()
    assert sorted(stats["pipes"]) == sorted(fuzz_axis.PIPE_ROWS)
    thin = {k: n for k, n in stats["pipes"].items() if n < 3}
    assert not thin, thin
    assert stats["pipes"]["dropped mode"] == fuzz_axis.SMOKE_CASES // 5


def test_no_operand_is_larger_than_2_20_elements():
    assert 0 < planned()["largest"] <= 1 << 20


def test_the_references_are_mostly_finite():
    """NaN handling has directed tests; the soak must not mostly compare NaN with NaN."""
    stats = planned()
    assert stats["float_cases"] > 0 and 3 * stats["nonfinite"] <= stats["float_cases"], (stats["nonfinite"], stats["float_cases"])


def test_the_cases_depend_on_count_and_seed_alone():
    lib = sma.load()
    a = [fuzz_axis.describe(c) for c in fuzz_axis.cases_of(60, 3, lib)]
    assert a == [fuzz_axis.describe(c) for c in fuzz_axis.cases_of(60, 3, lib)]
    assert a != [fuzz_axis.describe(c) for c in fuzz_axis.cases_of(60, 4, lib)]
