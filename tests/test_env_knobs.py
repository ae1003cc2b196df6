"""The inventory of environment switches: what the library's sources read is what INTEGRATION.md's table documents.

A variable read with getenv under simplemath_amd/csrc or include but missing from the table is an undocumented switch; a row
of the table that no source reads is a stale one.  Either way the inventory has drifted -- no device involved."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE_DIRS = (os.path.join(ROOT, "simplemath_amd", "csrc"), os.path.join(ROOT, "include"))
SOURCE_SUFFIXES = (".hip", ".h", ".hpp", ".cpp")  # (the generated jit_sources.inc repeats bcast_kernels.hip.h)
ELSEWHERE = ("Python binding only", "`bench.py` only")  # rows about variables that the C++ sources do not read


def variables_read_by_the_sources():
    names = set()
    for top in SOURCE_DIRS:
        for dirpath, _, files in os.walk(top):
            for f in files:
                if f.endswith(SOURCE_SUFFIXES):
                    with open(os.path.join(dirpath, f), encoding="utf-8") as fh:
                        names.update(re.findall(r'getenv\(\s*"(SMHIP_[A-Z0-9_]+)"', fh.read()))
    return names


def variables_in_the_table():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        text = fh.read()
    section = text[text.index("Environment switches"):]
    names, rows = set(), 0
    for line in section.splitlines():
        if line.startswith("#") and rows:
            break  # the next section
        cells = re.split(r"(?<!\\)\|", line)
        if len(cells) < 4 or not line.startswith("|") or set(cells[1].strip()) <= set("-: ") or cells[1].strip() == "variable":
            continue
        rows += 1
        if any(mark in "|".join(cells[2:]) for mark in ELSEWHERE):  # (an effect cell may hold bare pipes of its own)
            continue
        found = re.findall(r"SMHIP_[A-Z0-9_]+", cells[1])
        assert found, f"a row of the environment table names no variable: {line[:80]}"
        names.update(found)
    assert rows, "INTEGRATION.md: the environment table was not found"
    return names


def test_sources_and_table_list_the_same_variables():
    read, documented = variables_read_by_the_sources(), variables_in_the_table()
    assert read, "no getenv(\"SMHIP_...\") found under simplemath_amd/csrc and include"
    assert read - documented == set(), f"read by the sources, missing from INTEGRATION.md's table: {sorted(read - documented)}"
    assert documented - read == set(), f"in INTEGRATION.md's table, read by no source: {sorted(documented - read)}"
