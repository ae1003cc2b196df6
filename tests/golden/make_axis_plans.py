#!/usr/bin/env python3
"""Record what the three host-only axis planners answer: tests/golden/axis_plans.json.

    python -m simplemath_amd.build && python -m tests.golden.make_axis_plans

smhip_reduce_plan, smhip_scan_plan and smhip_argreduce_plan need no device, so the table pins the planners of whatever
library is built when this runs.  tests/test_axis_plans_host.py replays it: regenerate it only when a planner heuristic is
MEANT to change, and read the diff.

The case list is fixed and seedless (cases() below; the test checks that the table's inputs are exactly this list):

  the grid      ndim 1 .. 4, extents from EXTENTS (every product below 2^62), f32 and f64 (both vector widths), every
                axis -- for the reductions every non-empty mask -- and the layouts of layouts(): dense, all axes reversed
                (transposed), one axis stepped by 2, one axis of stride 0, a sub-block (row pitch larger than the row).
                The cross product is walked in mixed-radix order and every STRIDE[ndim]-th point kept (a prime, so the
                kept points run through every digit); the kind cycles with the point's number -- no plan depends on it.
  EXPLICIT      one named case per branch of a planner that the grid might miss.  Name -> what it reaches:
    reductions (reduce_axis.hip)
      row_g4 / row_g16 / row_g64 (+ _f64)   short rows, 4 / 16 / 64 lanes per row
      row_long / row_split                  a wave per row: 8192 rows are lanes enough; 4 rows of 2^26 are cut
      column / column_split                 (64, 2^20) over axis 0; (1000, 3000) over axis 0
      channel / channel_split               (1024, 4096, 3) over axis 1; (2^24, 3) over axis 0
      fill / none / gather                  sum over an empty extent; an empty result; reduced extents all 1
      two_groups / three_groups             axes 0, 2 of three; axes 0, 2, 4 of five (one pass per reduced group)
      copy_stride0 / copy_unmerged          a broadcast axis; a (4, 5, 6) array as .transpose(1, 0, 2) over its last axis
      transposed                            A.T over axis 0: the ROW walk, no copy
    scans (scan_axis.hip)
      copyonly                              R = 1
      row_g4 / row_g16 / row_g64            short rows
      row_long / row_split                  1024 rows; 4 rows of 2^26
      row_rows_1023 / _1024 / _1025         kRowSplitBelowRows = 1024: split below it only
      row_tile_8191 / _8192 / _8193         a chunk is at least a tile (4096 f32): R / tile = 1, 2, 2
      row_max_chunks                        one row of 2^24: 1024 chunks wanted, kRowMaxChunks = 256 taken
      column / column_split                 (4096, 4096) over axis 0; (70001, 8) over axis 0
      column_groups_63 / _64 / _65          kColumnSplitBelowGroups = 64 workgroups: split below it only
      column_block_511 / _512 / _513 (+ _f64_255 / _256)   a chunk is at least a block (256 rows f32, 128 f64)
      column_max_chunks                     (2^24, 8) over axis 0: kColumnMaxChunks = 1024 chunks
      copy_transposed / copy_stride0 / copy_subblock        every view is copied dense first
    argmax / argmin (argreduce_axis.hip)
      row_g4 / row_g16 / row_g64            short rows
      row_long / row_split                  (4096, 4096) over axis 1; (65, 4097) over axis 1: five chunks of 1024
      column / column_split                 (64, 2^20) over axis 0; (1000, 257) over axis 0
      two_finishing (+ _f64)                (2^24, 3) over axis 0: more than 4096 chunks, two finishing launches
      clamp_row / clamp_column              R = 2^33: lanes enough, still cut where a chunk's positions leave 32 bits
      r1 / r1_row / r1_copy                 an axis of one element
      copy_stride0 / copy_unmerged / copy_split / transposed / subblock / none
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "axis_plans.json")

EXTENTS = [1, 2, 3, 5, 8, 9, 16, 17, 64, 65, 255, 257, 1024, 4097, 1 << 16, (1 << 20) + 1, 1 << 24, 1 << 33]
LIMIT = 1 << 62
STRIDE = {1: 1, 2: 29, 3: 2003, 4: 120011}
DTYPES = ("f32", "f64")
KINDS = {"reduce": ("sum", "mean", "max", "min"), "scan": ("cumsum", "cumprod", "cummax", "cummin"), "argreduce": ("argmax", "argmin")}


def dense(shape):
    st, acc = [], 1
    for e in reversed(shape):
        st.append(acc)
        acc *= e
    return st[::-1]


def layouts(shape):
    """The strides (elements) of the layouts of one shape, in a fixed order; None where a layout is the dense one again."""
    nd = len(shape)
    out = [dense(shape)]
    out.append(dense(shape[::-1])[::-1] if nd > 1 else None)  # all axes reversed: the transposed view of the reversed shape
    for k in range(nd):  # axis k stepped by 2: every second index of an axis twice as long
        out.append([s * 2 if d <= k else s for d, s in enumerate(dense(shape))])
    for k in range(nd):  # axis k broadcast
        out.append([0 if d == k else s for d, s in enumerate(dense(shape[:k] + [1] + shape[k + 1:]))])
    out.append(dense(shape[:-1] + [shape[-1] + 3]) if nd > 1 else None)  # rows of a wider array
    return out


def calls(nd):
    """(family, axis or axes) of one operand: every non-empty mask for the reductions, every axis for the others."""
    out = [("reduce", [d for d in range(nd) if m >> d & 1]) for m in range(1, 1 << nd)]
    return out + [(fam, d) for fam in ("scan", "argreduce") for d in range(nd)]


def grid():
    for nd in range(1, 5):
        nl, nc, ne = 3 + 2 * nd, len(calls(nd)), len(EXTENTS)
        total = ne ** nd * nl * len(DTYPES) * nc
        for n in range(0, total, STRIDE[nd]):
            q, c = divmod(n, nc)
            q, t = divmod(q, len(DTYPES))
            q, li = divmod(q, nl)
            shape = []
            for _ in range(nd):
                q, e = divmod(q, ne)
                shape.append(EXTENTS[e])
            prod = 1
            for e in shape:
                prod *= e
            strides = layouts(shape)[li]
            if prod >= LIMIT or strides is None:
                continue
            fam, axis = calls(nd)[c]
            yield fam, KINDS[fam][n % len(KINDS[fam])], DTYPES[t], shape, strides, axis


T = True  # strides: the transposed view
EXPLICIT = [  # name, family, dtype, shape, strides (None: dense), axis or axes
    ("row_g4", "reduce", "f32", [1000, 13], None, [1]),
    ("row_g16", "reduce", "f32", [1000, 50], None, [1]),
    ("row_g64", "reduce", "f32", [1000, 200], None, [1]),
    ("row_g4_f64", "reduce", "f64", [1000, 5], None, [1]),
    ("row_g16_f64", "reduce", "f64", [1000, 31], None, [1]),
    ("row_g64_f64", "reduce", "f64", [1000, 100], None, [1]),
    ("row_long", "reduce", "f32", [8192, 3000], None, [1]),
    ("row_split", "reduce", "f32", [4, 1 << 26], None, [1]),
    ("row_split_f64", "reduce", "f64", [4, 1 << 26], None, [1]),
    ("column", "reduce", "f32", [64, 1 << 20], None, [0]),
    ("column_split", "reduce", "f32", [1000, 3000], None, [0]),
    ("channel", "reduce", "f32", [1024, 4096, 3], None, [1]),
    ("channel_split", "reduce", "f32", [1 << 24, 3], None, [0]),
    ("channel_split_f64", "reduce", "f64", [64, 224, 224, 3], None, [0, 1, 2]),
    ("fill", "reduce", "f32", [3, 0, 4], None, [1]),
    ("none", "reduce", "f32", [3, 0, 4], None, [0]),
    ("gather", "reduce", "f32", [3, 1, 4], None, [1]),
    ("two_groups", "reduce", "f32", [50, 60, 70], None, [0, 2]),
    ("two_groups_split", "reduce", "f32", [4097, 3, 4097], None, [0, 2]),
    ("three_groups", "reduce", "f32", [5, 6, 7, 8, 9], None, [0, 2, 4]),
    ("three_groups_f64", "reduce", "f64", [2000, 2, 300, 3, 65], None, [0, 2, 4]),
    ("copy_stride0", "reduce", "f32", [8, 5], [0, 1], [1]),
    ("copy_unmerged", "reduce", "f32", [5, 4, 6], [6, 30, 1], [2]),
    ("transposed", "reduce", "f32", [8192, 16384], T, [0]),
    ("copyonly", "scan", "f32", [3, 1, 4], None, 1),
    ("row_g4", "scan", "f32", [1000, 13], None, 1),
    ("row_g16", "scan", "f32", [1000, 50], None, 1),
    ("row_g64", "scan", "f64", [1000, 100], None, 1),
    ("row_long", "scan", "f32", [1024, 1 << 20], None, 1),
    ("row_split", "scan", "f32", [4, 1 << 26], None, 1),
    ("row_rows_1023", "scan", "f32", [1023, 1 << 16], None, 1),
    ("row_rows_1024", "scan", "f32", [1024, 1 << 16], None, 1),
    ("row_rows_1025", "scan", "f32", [1025, 1 << 16], None, 1),
    ("row_tile_8191", "scan", "f32", [4, 8191], None, 1),
    ("row_tile_8192", "scan", "f32", [4, 8192], None, 1),
    ("row_tile_8193", "scan", "f32", [4, 8193], None, 1),
    ("row_tile_f64_4095", "scan", "f64", [4, 4095], None, 1),
    ("row_tile_f64_4096", "scan", "f64", [4, 4096], None, 1),
    ("row_max_chunks", "scan", "f32", [1 << 24], None, 0),
    ("column", "scan", "f32", [4096, 4096], None, 0),
    ("column_split", "scan", "f32", [70001, 8], None, 0),
    ("column_groups_63", "scan", "f32", [63, 4096, 64], None, 1),
    ("column_groups_64", "scan", "f32", [64, 4096, 64], None, 1),
    ("column_groups_65", "scan", "f32", [65, 4096, 64], None, 1),
    ("column_block_511", "scan", "f32", [511, 64], None, 0),
    ("column_block_512", "scan", "f32", [512, 64], None, 0),
    ("column_block_513", "scan", "f32", [513, 64], None, 0),
    ("column_block_f64_255", "scan", "f64", [255, 64], None, 0),
    ("column_block_f64_256", "scan", "f64", [256, 64], None, 0),
    ("column_max_chunks", "scan", "f32", [1 << 24, 8], None, 0),
    ("copy_transposed", "scan", "f32", [100, 50], T, 1),
    ("copy_stride0", "scan", "f32", [8, 5], [0, 1], 0),
    ("copy_subblock", "scan", "f32", [8, 5], [16, 1], 0),
    ("copy_split", "scan", "f32", [300, 70001], T, 1),
    ("none", "scan", "f32", [3, 0, 4], None, 1),
    ("row_g4", "argreduce", "f32", [1000, 13], None, 1),
    ("row_g16", "argreduce", "f32", [1000, 50], None, 1),
    ("row_g64", "argreduce", "f64", [1000, 100], None, 1),
    ("row_long", "argreduce", "f32", [4096, 4096], None, 1),
    ("row_split", "argreduce", "f32", [65, 4097], None, 1),
    ("row_split_one", "argreduce", "f32", [(1 << 31) + 5], None, 0),
    ("column", "argreduce", "f32", [64, 1 << 20], None, 0),
    ("column_split", "argreduce", "f32", [1000, 257], None, 0),
    ("two_finishing", "argreduce", "f32", [1 << 24, 3], None, 0),
    ("two_finishing_f64", "argreduce", "f64", [1 << 20, 4], None, 0),
    ("clamp_row", "argreduce", "f32", [1 << 19, 1 << 33], None, 1),
    ("clamp_column", "argreduce", "f32", [(1 << 33) + 1, 1 << 20], None, 0),
    ("r1", "argreduce", "f32", [3, 1, 4], None, 1),
    ("r1_row", "argreduce", "f32", [1], None, 0),
    ("r1_copy", "argreduce", "f32", [5, 1], [3, 7], 1),
    ("copy_stride0", "argreduce", "f32", [8, 5], [0, 1], 0),
    ("copy_unmerged", "argreduce", "f32", [5, 4, 6], [6, 30, 1], 2),
    ("copy_split", "argreduce", "f32", [3, 70001], [140002, 2], 1),
    ("transposed", "argreduce", "f32", [4097, 65], T, 0),
    ("subblock", "argreduce", "f32", [8, 5], [16, 1], 1),
    ("none", "argreduce", "f32", [3, 0, 4], None, 0),
]


def cases():
    """Every case of the table, in its order: (family, kind, dtype, shape, strides, axis or axes)."""
    out = []
    for _, fam, dt, shape, strides, axis in EXPLICIT:
        st = dense(shape) if strides is None else dense(shape[::-1])[::-1] if strides is T else strides
        out.append((fam, KINDS[fam][0], dt, shape, st, axis))
    out.extend(grid())
    return out


def answer(lib, case):
    """The case with what the built library's planner says: + route word, launches, [O, R, I] (and the chunk)."""
    fam, kind, dt, shape, strides, axis = case
    dtype = {"f32": "float32", "f64": "float64"}[dt]
    got = {"reduce": lib.reduce_plan, "scan": lib.scan_plan, "argreduce": lib.argreduce_plan}[fam](kind, dtype, shape, strides, tuple(axis) if fam == "reduce" else axis)
    return [fam, kind, dt, shape, strides, axis, got[0], got[1], list(got[2])] + list(got[3:])


def main():
    sys.path.insert(0, ROOT)
    import simplemath_amd as sma
    lib = sma.load()
    rows = [answer(lib, c) for c in cases()]
    text = "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n"
    with open(TABLE, "w") as f:
        f.write(text)
    print("%s: %d rows, %d bytes (%s)" % (TABLE, len(rows), len(text), lib.version()))


if __name__ == "__main__":
    main()
