"""The shapes of the tests past 2^31 elements and 4 GiB, in one place (a plain module, not a test).

test_past_2p31_host.py pins every case's plan (route word, launches) and the size arithmetic it exists for on the CPU;
test_past_2p31_gpu.py runs exactly these shapes on the device.  Strides are in elements.  A case names
  sort      dtype, shape, strides, axis                                     -> lib.sort_plan
  take      dtype, a_strides, R, idx_strides, out, axis                     -> lib.take_plan
  scatter   dtype, out, axis, idx_strides, val_strides, J, unique           -> lib.scatter_plan
and what it is for: `large` (the elements of the operand or result that is large, with `itemsize` its bytes each), `entries`
(what the kernel's flat entry counter runs to) and the plan expected, (route, flags, launches).

The sizes:
  LINES x 1000        2^31 + 16 352 elements: 16 whole lines lie past element 2^31                              S1 T3 C5
  262 129 x 8193      2^31 + 139 249: three tiles a line, two merge passes                                      S2
  257 x 8 355 984     sorted along axis 0: a skinny transposed copy in and out; 3 x 715 829 250: a record-shaped one   S3 S3b
  TABLE_ROWS x 1024   2^31 + 5120 elements: rows 2^21 .. 2^21 + 4 lie past element 2^31, row 2^20 starts at byte 2^32   T1 T2 C1-C3
  FLAT                2^31 + 4099 elements in one axis: positions that do not fit 32 bits                       T5 C4
  WIDE_ROWS x 1031    2^32 + 100 348 entries with an inner extent of 1031: the flat entry counter passes 2^32 while the
                      divisor stays small, so div_small goes from its 32-bit to its 64-bit branch inside one launch   T4 C6"""
import numpy as np

import simplemath_amd as sma

P31, P32, P33 = 1 << 31, 1 << 32, 1 << 33

LINES, LINE = 2_147_500, 1000                 # S1, T3, C5
S2_LINES, S2_LINE = 262_129, 8193
S3_ROWS, S3_COLS = 257, 8_355_984
S3B_ROWS, S3B_COLS = 3, 715_829_250
TABLE_ROWS, TABLE_COLS = (1 << 21) + 5, 1024  # T1, T2, C1 - C3
FLAT = P31 + 4099                             # T5, C4
WIDE_ROWS, WIDE_COLS, WIDE_R = 4_165_924, 1031, 7   # T4, C6
T1_IDS, C1_IDS, C2_IDS, C4_IDS, C5_ENTRIES = 4096, 300, 3000, 5000, 1500

f32, i64 = np.dtype(np.float32), np.dtype(np.int64)

_SORT = dict(ROW=sma.SORT_ROUTE_ROW, MERGE=sma.SORT_MERGE, COPY=sma.SORT_COPY)
_TAKE = dict(LINE=sma.TAKE_ROUTE_LINE, ROWS=sma.TAKE_ROUTE_ROWS, DIRECT=sma.TAKE_ROUTE_DIRECT, COPY=sma.TAKE_COPY)
_SCATTER = dict(DIRECT=sma.SCATTER_ROUTE_DIRECT, ROWS=sma.SCATTER_ROUTE_ROWS, SORTED=sma.SCATTER_ROUTE_SORTED, SORTED_ROWS=sma.SCATTER_ROUTE_SORTED_ROWS,
                COPY=sma.SCATTER_COPY)


def _word(names, text):
    word = 0
    for part in text.split("|"):
        word |= names[part]
    return word


def _sort(dtype, shape, axis, plan, launches):
    shape = list(shape)
    strides = [int(np.prod(shape[d + 1:], dtype=np.int64)) for d in range(len(shape))]
    n = int(np.prod(shape, dtype=np.int64))
    return dict(family="sort", dtype=np.dtype(dtype), shape=shape, strides=strides, axis=axis, plan=_word(_SORT, plan), launches=launches, large=n,
                itemsize=np.dtype(dtype).itemsize, entries=n)


def _take(dtype, a_strides, R, idx_strides, out, axis, plan, large):
    return dict(family="take", dtype=np.dtype(dtype), a_strides=list(a_strides), R=R, idx_strides=list(idx_strides), out=list(out), axis=axis,
                plan=_word(_TAKE, plan), launches=1, large=large, itemsize=np.dtype(dtype).itemsize, entries=int(np.prod(out, dtype=np.int64)))


def _scatter(dtype, out, axis, idx_strides, val_strides, J, unique, plan, launches):
    walk = [J if d == axis else n for d, n in enumerate(out)]
    return dict(family="scatter", dtype=np.dtype(dtype), out=list(out), axis=axis, idx_strides=list(idx_strides), val_strides=list(val_strides), J=J,
                unique=unique, plan=_word(_SCATTER, plan), launches=launches, large=int(np.prod(out, dtype=np.int64)), itemsize=np.dtype(dtype).itemsize,
                entries=int(np.prod(walk, dtype=np.int64)))


CASES = {
    # ---- sort: launches are those of a call that asks for both outputs, not in place
    "S1": _sort(f32, (LINES, LINE), 1, "ROW", 1),
    "S1_i64": _sort(i64, (LINES, LINE // 2), 1, "ROW", 1),          # the same buffer as eight-byte elements
    "S2": _sort(f32, (S2_LINES, S2_LINE), 1, "ROW|MERGE", 3),
    "S3": _sort(f32, (S3_ROWS, S3_COLS), 0, "ROW|COPY", 4),
    "S3b": _sort(f32, (S3B_ROWS, S3B_COLS), 0, "ROW|COPY", 4),
    # ---- take
    "T1": _take(f32, (TABLE_COLS, 1), TABLE_ROWS, (1, 0), (T1_IDS, TABLE_COLS), 0, "ROWS", TABLE_ROWS * TABLE_COLS),
    "T1_i64": _take(i64, (TABLE_COLS // 2, 1), TABLE_ROWS, (1, 0), (T1_IDS, TABLE_COLS // 2), 0, "ROWS", TABLE_ROWS * TABLE_COLS // 2),
    "T2": _take(f32, (TABLE_COLS, 1), TABLE_ROWS, (TABLE_COLS, 1), (8, TABLE_COLS), 0, "DIRECT", TABLE_ROWS * TABLE_COLS),
    "T3": _take(f32, (LINE, 1), LINE, (0, 1), (LINES, LINE), 1, "LINE", LINES * LINE),
    "T4": _take(f32, (WIDE_COLS, 1), WIDE_R, (0, 1), (WIDE_ROWS, WIDE_COLS), 0, "DIRECT", WIDE_ROWS * WIDE_COLS),
    "T5": _take(f32, (1,), FLAT, (1,), (T1_IDS,), 0, "DIRECT", FLAT),
    # ---- scatter
    "C1": _scatter(f32, (TABLE_ROWS, TABLE_COLS), 0, (1, 0), (TABLE_COLS, 1), C1_IDS, True, "ROWS", 1),
    "C2": _scatter(f32, (TABLE_ROWS, TABLE_COLS), 0, (1, 0), (TABLE_COLS, 1), C2_IDS, False, "SORTED_ROWS", 3),
    "C3_unique": _scatter(f32, (TABLE_ROWS, TABLE_COLS), 0, (TABLE_COLS, 1), (TABLE_COLS, 1), 8, True, "DIRECT", 1),
    "C3": _scatter(f32, (TABLE_ROWS, TABLE_COLS), 0, (TABLE_COLS, 1), (TABLE_COLS, 1), 24, False, "SORTED", 3),
    "C4": _scatter(f32, (FLAT,), 0, (1,), (1,), C4_IDS, False, "SORTED", 4),
    "C5": _scatter(f32, (LINES, LINE), 1, (0, 1), (0, 1), C5_ENTRIES, False, "SORTED", 3),
    "C6": _scatter(f32, (WIDE_ROWS, 1, WIDE_COLS), 1, (0, 0, 1), (0, 0, 1), 1, False, "DIRECT", 1),
}

# The variant of T4 that must NOT be used: with a middle axis of 5 the walk does not come to three axes in place, and the plan
# copies the broadcast operand dense first -- (833185, 7, 1031) f32, 24 GiB.
T4_TRAP = _take(f32, (0, WIDE_COLS, 1), WIDE_R, (0, WIDE_COLS, 1), (833_185, 5, WIDE_COLS), 1, "DIRECT|COPY", 833_185 * WIDE_R * WIDE_COLS)


def plan_of(lib, case):
    """(route word, launches) of a case through the library's own planner (host only)."""
    c = case
    if c["family"] == "sort":
        return lib.sort_plan(c["dtype"], c["shape"], c["strides"], c["axis"])[:2]
    if c["family"] == "take":
        return lib.take_plan(c["dtype"], c["a_strides"], c["R"], c["idx_strides"], c["out"], c["axis"])[:2]
    return lib.scatter_plan(c["dtype"], c["out"], c["axis"], c["idx_strides"], c["val_strides"], c["J"], unique=c["unique"])[:2]


def boundary_lines(lines, R, itemsizes):
    """The lines of a dense [lines][R] array that a test samples, ascending and without repeats:
      the first line and the line after it;
      the line holding element 2^31 and the line on each side of it;
      for each item size, the lines holding byte offsets 2^32 and 2^33 and the line on each side of each;
      16 lines spread evenly over the range past element 2^31 (all of them where there are no more);
      the last two lines.
    What the array does not reach is left out."""
    want = {0, 1, lines - 2, lines - 1}
    holders = [P31 // R]
    for size in itemsizes:
        holders += [P32 // size // R, P33 // size // R]
    for line in holders:
        want |= {line - 1, line, line + 1}
    first_past = P31 // R + 1
    if first_past < lines:
        count = min(16, lines - first_past)
        want |= {first_past + (k * (lines - 1 - first_past)) // max(count - 1, 1) for k in range(count)}
    return sorted(line for line in want if 0 <= line < lines)
