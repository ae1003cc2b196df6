#!/usr/bin/env python3
"""Record what the C ABI's entry points answer to calls they refuse: tests/golden/abi_errors.json.

    python -m simplemath_amd.build && python -m tests.golden.make_abi_errors

RUN THIS ON A MACHINE WITHOUT A DEVICE.  The device pointers below are made-up integers; a row is kept only when the library
answers SMHIP_OK, SMHIP_ERR_INVALID or SMHIP_ERR_UNSUPPORTED, and without a device every call that gets past an entry point's
checks ends in SMHIP_ERR_NO_DEVICE -- the generator stops there and names the row, so nothing recorded ever reaches a launch.
tests/test_abi_errors_host.py replays the table against the built library and compares return code and message for equality:
which check fires first and its full text are the contract.  Regenerate it only when a refusal is MEANT to change, and read the
diff.

The case list is fixed (cases() below; the test checks that the table's inputs are exactly this list).  A row is
[method of the binding, case name, keyword arguments, return code, message]; the scalars of where / select (`rhs`, `a_scalar`,
`b_scalar`) are recorded as a number and handed over as a host array of one element.  Every entry point has one well-formed base
call -- (8,) or (3, 5), f32 and i64, pointers 1 MiB apart -- and the cases are that call with one fault (or two, to pin which
message wins): see one_fault() for the list.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "abi_errors.json")

OK, INVALID, UNSUPPORTED = 0, -1, -4
F32, F64, I32, I64 = range(4)
ESZ = {F32: 4, F64: 8, I32: 4, I64: 8}
# stand-ins for device pointers: well separated, 16-byte aligned, never dereferenced
A, B, C, D, E, F, G, H = (k << 20 for k in range(1, 9))
SCALARS = ("rhs", "a_scalar", "b_scalar")


def dense(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.insert(0, acc)
        acc *= d
    return st


def span(shape, strides, esz):
    """Bytes from a view's first element to its last."""
    return (sum((e - 1) * s for e, s in zip(shape, strides)) + 1) * esz


def count(shape):
    n = 1
    for e in shape:
        n *= e
    return n


def one_fault(fn, base, *, enums=(), dtypes=("dtype",), shape=None, strides=(), axis=None, ptrs=(), aligned=(), ndim_kw=True, overlaps=(),
              in_place=None, empty=None, plan=False, values=True):
    """The cases of one entry point: (method, case name, keyword arguments).

    enums      keys of enum arguments: each gets -1 and 99
    dtypes     keys of dtype arguments: each gets -1 and 4
    shape      key of the shape: ndim 0 and 7, null, a negative extent
    strides    keys of stride arrays (all follow the shape to ndim 0 / 7): each null, each with a negative stride
    axis       key of the axis: -1 and ndim
    ptrs       keys of pointers the base call gives: each null in turn
    aligned    keys of pointers whose alignment the entry point checks: each one byte off in turn
    overlaps   (key of the written span, its bytes, key of the other span, its bytes, bytes of one element): the written span moved
               over the other one's first and over its last element
    in_place   (key of the result, key of the operand, key of the operand's strides): the same pointer with the operand stepped,
               broadcast and transposed
    empty      the overrides of the call that has nothing to do (an empty shape, every pointer null): SMHIP_OK
    values     False leaves out the faults in the enums, dtypes, shape, strides and axis (they do not depend on the element type)
    then two faults at once: a bad dtype with a null buffer, a negative stride with an overlap, misaligned with overlapping.
    """
    def case(name, **over):
        kw = dict(base)
        kw.update(over)
        return (fn, name, kw)

    def with_ndim(over, nd):
        if ndim_kw and not plan:
            over["ndim"] = nd
        return over

    def negated(v):
        return [-1 if v[0] == 0 else -v[0]] + list(v[1:])

    out = []
    for k in enums if values else ():
        out += [case("%s=-1" % k, **{k: -1}), case("%s=99" % k, **{k: 99})]
    for k in dtypes if values else ():
        out += [case("%s=-1" % k, **{k: -1}), case("%s=4" % k, **{k: 4})]
    if shape and values:
        nd = len(base[shape])
        out.append(case("ndim=0", **with_ndim({shape: [], **{k: [] for k in strides}}, 0)))
        out.append(case("ndim=7", **{shape: [2] * 7, **{k: dense([2] * 7) for k in strides}}))
        if axis:
            out += [case("axis=-1", **{axis: -1}), case("axis=ndim", **{axis: nd})]
        if not plan:
            out.append(case("null shape", **with_ndim({shape: None}, nd)))
            out += [case("null %s" % k, **{k: None}) for k in strides]
        out.append(case("negative extent", **{shape: negated(base[shape])}))
        out += [case("negative %s" % k, **{k: negated(base[k])}) for k in strides]
    null = {k: None if k in SCALARS else 0 for k in ptrs}
    out += [case("null %s" % k, **{k: null[k]}) for k in ptrs]
    out += [case("misaligned %s" % k, **{k: base[k] + 1}) for k in aligned]
    for w, w_bytes, o, o_bytes, unit in overlaps:
        out.append(case("%s over the front of %s" % (w, o), **{w: base[o] - w_bytes + unit}))
        out.append(case("%s over the back of %s" % (w, o), **{w: base[o] + o_bytes - unit}))
    if in_place:
        res, opd, st = in_place
        for name, shp, s in (("stepped", [8], [2]), ("broadcast", [8], [0]), ("transposed", [4, 4], [1, 4])):
            over = {shape: shp, res: base[opd], **{k: dense(shp) for k in strides}}
            over[st] = s
            if axis:
                over[axis] = 0
            out.append(case("%s is %s, %s" % (res, opd, name), **over))
    if empty is not None:
        out.append(case("nothing to do", **empty))
    if dtypes and ptrs and values:
        out.append(case("bad dtype and null %s" % ptrs[0], **{dtypes[0]: 4, ptrs[0]: null[ptrs[0]]}))
    if strides and overlaps:
        w, w_bytes, o, o_bytes, unit = overlaps[0]
        out.append(case("negative %s and %s over %s" % (strides[0], w, o), **{strides[0]: negated(base[strides[0]]), w: base[o] + o_bytes - unit}))
    if aligned and overlaps:
        w, w_bytes, o, o_bytes, unit = overlaps[0]
        out.append(case("%s misaligned and over %s" % (w, o), **{w: base[o] + 1}))
    return out


def raw_cases(dt):
    """The entry points that launch, on element type `dt` (F32 or I64)."""
    e, w = ESZ[dt], 8
    s35, s8 = [3, 5], [8]
    out = []

    def faults(fn, base, **kw):  # the faults in plain values are recorded once, with f32
        return one_fault(fn, base, values=dt == F32, **kw)

    # ---- the axis families (no alignment checks)
    base = dict(kind=0, dtype=dt, a_ptr=A, shape=s35, strides=[5, 1], mask=2, out_ptr=B)
    out += faults("reduce_raw", base, enums=["kind"], shape="shape", strides=["strides"], ptrs=["a_ptr", "out_ptr"], ndim_kw=False,
                     empty=dict(shape=[0, 5], a_ptr=0, out_ptr=0))
    out += [("reduce_raw", "no axis", dict(base, mask=0)), ("reduce_raw", "an axis outside", dict(base, mask=4))]

    base = dict(kind=0, dtype=dt, a_ptr=A, shape=s35, strides=[5, 1], axis=1, out_ptr=B)
    out += faults("scan_raw", base, enums=["kind"], shape="shape", strides=["strides"], axis="axis", ptrs=["a_ptr", "out_ptr"],
                     overlaps=[("out_ptr", 15 * e, "a_ptr", 15 * e, e)], in_place=("out_ptr", "a_ptr", "strides"), empty=dict(shape=[3, 0], a_ptr=0, out_ptr=0))

    base = dict(kind=0, dtype=dt, a_ptr=A, shape=s35, strides=[5, 1], axis=1, index_ptr=B, value_ptr=C)
    out += faults("argreduce_raw", base, enums=["kind"], shape="shape", strides=["strides"], axis="axis", ptrs=["a_ptr", "index_ptr"],
                     overlaps=[("index_ptr", 3 * w, "a_ptr", 15 * e, w), ("value_ptr", 3 * e, "a_ptr", 15 * e, e), ("index_ptr", 3 * w, "value_ptr", 3 * e, w)],
                     empty=dict(shape=[0, 5], a_ptr=0, index_ptr=0, value_ptr=0))
    out.append(("argreduce_raw", "an empty axis", dict(base, shape=[3, 0])))

    base = dict(order=0, dtype=dt, a_ptr=A, shape=s35, strides=[5, 1], axis=1, values_ptr=B, index_ptr=C)
    out += faults("sort_raw", base, enums=["order"], shape="shape", strides=["strides"], axis="axis", ptrs=["a_ptr"],
                     overlaps=[("values_ptr", 15 * e, "a_ptr", 15 * e, e), ("index_ptr", 15 * w, "a_ptr", 15 * e, w), ("index_ptr", 15 * w, "values_ptr", 15 * e, w)],
                     in_place=("values_ptr", "a_ptr", "strides"), empty=dict(shape=[3, 0], a_ptr=0, values_ptr=0, index_ptr=0))
    out.append(("sort_raw", "no result", dict(base, values_ptr=0, index_ptr=0)))
    out.append(("sort_raw", "a transposed operand, index_ptr over it", dict(base, shape=[4, 4], strides=[1, 4], index_ptr=A + 8)))

    base = dict(mode=0, dtype=dt, a_ptr=A, a_strides=[7, 1], a_extent=7, idx_ptr=B, idx_strides=[5, 1], out_shape=s35, axis=1, out_ptr=C, bad_ptr=D)
    out += faults("take_raw", base, enums=["mode"], shape="out_shape", strides=["a_strides", "idx_strides"], axis="axis", ptrs=["a_ptr", "idx_ptr", "out_ptr"],
                     overlaps=[("out_ptr", 15 * e, "a_ptr", 21 * e, e), ("out_ptr", 15 * e, "idx_ptr", 15 * w, w), ("out_ptr", 15 * e, "bad_ptr", w, e),
                               ("bad_ptr", w, "a_ptr", 21 * e, w), ("bad_ptr", w, "idx_ptr", 15 * w, w)],
                     empty=dict(out_shape=[3, 0], a_ptr=0, idx_ptr=0, out_ptr=0, bad_ptr=0))
    out.append(("take_raw", "a negative extent of a", dict(base, a_extent=-1)))
    out.append(("take_raw", "nothing to take from", dict(base, a_extent=0)))
    out.append(("take_raw", "a transposed operand, out_ptr over it", dict(base, a_strides=[1, 3], out_ptr=A + 20 * e)))

    base = dict(kind=0, mode=0, flags=0, dtype=dt, out_ptr=A, out_shape=s35, axis=1, idx_ptr=B, idx_strides=[4, 1], val_ptr=C, val_strides=[4, 1], n_entries=4, bad_ptr=D)
    out += faults("scatter_raw", base, enums=["kind", "mode", "flags"], shape="out_shape", strides=["idx_strides", "val_strides"], axis="axis",
                     ptrs=["out_ptr", "idx_ptr", "val_ptr"],
                     overlaps=[("out_ptr", 15 * e, "idx_ptr", 12 * w, w), ("out_ptr", 15 * e, "val_ptr", 12 * e, e), ("out_ptr", 15 * e, "bad_ptr", w, e),
                               ("bad_ptr", w, "idx_ptr", 12 * w, w), ("bad_ptr", w, "val_ptr", 12 * e, w)],
                     empty=dict(n_entries=0, out_ptr=0, idx_ptr=0, val_ptr=0, bad_ptr=0))
    out.append(("scatter_raw", "a negative number of entries", dict(base, n_entries=-1)))
    out.append(("scatter_raw", "broadcast values, out_ptr over the one element", dict(base, val_strides=[0, 0], out_ptr=C - 14 * e)))

    # ---- counting (pointers checked for alignment)
    base = dict(side=0, dtype=dt, edges_ptr=A, n_edges=5, x_ptr=B, shape=s8, strides=[1], out_ptr=C)
    out += faults("searchsorted_raw", base, enums=["side"], shape="shape", strides=["strides"], ptrs=["edges_ptr", "x_ptr", "out_ptr"], aligned=["edges_ptr", "x_ptr", "out_ptr"],
                     overlaps=[("out_ptr", 8 * w, "x_ptr", 8 * e, w), ("out_ptr", 8 * w, "edges_ptr", 5 * e, w)], empty=dict(shape=[0], edges_ptr=0, x_ptr=0, out_ptr=0))
    out.append(("searchsorted_raw", "a negative number of edges", dict(base, n_edges=-1)))
    out.append(("searchsorted_raw", "a transposed operand, out_ptr over it", dict(base, shape=[4, 4], strides=[1, 4], out_ptr=B + 8)))

    ids = dt if dt == I64 else I32  # bincount counts integers
    base = dict(mode=0, dtype=ids, ids_ptr=A, shape=s8, strides=[1], nbins=6, counts_ptr=B, bad_ptr=C)
    out += faults("bincount_raw", base, enums=["mode"], shape="shape", strides=["strides"], ptrs=["ids_ptr", "counts_ptr"], aligned=["ids_ptr", "counts_ptr", "bad_ptr"],
                     overlaps=[("counts_ptr", 6 * w, "ids_ptr", 8 * ESZ[ids], w), ("counts_ptr", 6 * w, "bad_ptr", w, w), ("bad_ptr", w, "ids_ptr", 8 * ESZ[ids], w)],
                     empty=dict(shape=[0], nbins=0, ids_ptr=0, counts_ptr=0, bad_ptr=0))
    if dt == I64:
        out.append(("bincount_raw", "float ids", dict(base, dtype=F32)))
    out.append(("bincount_raw", "a negative number of bins", dict(base, nbins=-1)))
    out.append(("bincount_raw", "no ids, null counts", dict(base, shape=[0], ids_ptr=0, counts_ptr=0)))

    base = dict(flags=0, dtype=dt, x_ptr=A, shape=s8, strides=[1], edges_ptr=B, bins=4, lo=0.0, hi=1.0, counts_ptr=C)
    out += faults("histogram_raw", base, enums=["flags"], shape="shape", strides=["strides"], ptrs=["x_ptr", "edges_ptr", "counts_ptr"], aligned=["x_ptr", "edges_ptr", "counts_ptr"],
                     overlaps=[("counts_ptr", 4 * w, "x_ptr", 8 * e, w), ("counts_ptr", 4 * w, "edges_ptr", 5 * e, w)],
                     empty=dict(shape=[0], bins=0, x_ptr=0, edges_ptr=0, counts_ptr=0))
    out.append(("histogram_raw", "a negative number of bins", dict(base, bins=-1)))
    out.append(("histogram_raw", "uniform, the range reversed", dict(base, flags=1, lo=1.0, hi=0.0)))
    out.append(("histogram_raw", "uniform, no bins", dict(base, flags=1, bins=0)))
    # no elements: the table may be null while its length is not
    out.append(("histogram_raw", "no elements, a null table, counts at 8", dict(base, shape=[0], x_ptr=0, edges_ptr=0, counts_ptr=8)))
    out.append(("histogram_raw", "no elements, a null table, counts at 16", dict(base, shape=[0], x_ptr=0, edges_ptr=0, counts_ptr=16)))
    out.append(("histogram_raw", "no elements, a null table, null counts", dict(base, shape=[0], x_ptr=0, edges_ptr=0, counts_ptr=0)))

    # ---- one operand, one result
    base = dict(fn=0, dtype=dt, a_ptr=A, strides=[5, 1], shape=s35, out_ptr=B)
    out += faults("unary_raw", base, enums=["fn"], shape="shape", strides=["strides"], ptrs=["a_ptr", "out_ptr"], ndim_kw=False,
                     overlaps=[("out_ptr", 15 * e, "a_ptr", 15 * e, e)], in_place=("out_ptr", "a_ptr", "strides"), empty=dict(shape=[3, 0], a_ptr=0, out_ptr=0))
    if dt == I64:
        out.append(("unary_raw", "sqrt of integers", dict(base, fn=2)))
        out.append(("unary_raw", "sqrt of integers, null buffers", dict(base, fn=2, a_ptr=0, out_ptr=0)))

    dst = F64 if dt == F32 else I32
    base = dict(src_dtype=dt, dst_dtype=dst, a_ptr=A, strides=[5, 1], shape=s35, out_ptr=B)
    out += faults("convert_raw", base, dtypes=["src_dtype", "dst_dtype"], shape="shape", strides=["strides"], ptrs=["a_ptr", "out_ptr"], ndim_kw=False,
                     overlaps=[("out_ptr", 15 * ESZ[dst], "a_ptr", 15 * e, max(e, ESZ[dst]))], in_place=("out_ptr", "a_ptr", "strides"), empty=dict(shape=[3, 0], a_ptr=0, out_ptr=0))
    out.append(("convert_raw", "out_ptr is a_ptr, dense", dict(base, out_ptr=A)))

    # ---- choosing by condition (pointers checked for alignment)
    base = dict(cmp=5, dtype=dt, x_ptr=A, x_strides=[1], y_ptr=0, y_strides=None, rhs=1.0, a_ptr=B, a_strides=[1], a_scalar=None, b_ptr=C, b_strides=[1], b_scalar=None,
                shape=s8, out_ptr=D)
    out += faults("where_raw", base, enums=["cmp"], shape="shape", strides=["x_strides", "a_strides", "b_strides"], ptrs=["x_ptr", "a_ptr", "b_ptr", "out_ptr", "rhs"],
                     aligned=["x_ptr", "a_ptr", "b_ptr", "out_ptr"],
                     overlaps=[("out_ptr", 8 * e, "x_ptr", 8 * e, e), ("out_ptr", 8 * e, "a_ptr", 8 * e, e), ("out_ptr", 8 * e, "b_ptr", 8 * e, e)],
                     in_place=("out_ptr", "x_ptr", "x_strides"), empty=dict(shape=[0], x_ptr=0, a_ptr=0, b_ptr=0, out_ptr=0))
    with_y = dict(base, y_ptr=E, y_strides=[1], rhs=None)
    out += [("where_raw", "y: null strides", dict(with_y, y_strides=None)), ("where_raw", "y: a negative stride", dict(with_y, y_strides=[-1])),
            ("where_raw", "y: misaligned", dict(with_y, y_ptr=E + 1)), ("where_raw", "out_ptr over the front of y", dict(with_y, out_ptr=E - 7 * e)),
            ("where_raw", "out_ptr over the back of y", dict(with_y, out_ptr=E + 7 * e)),
            ("where_raw", "out_ptr is a_ptr, broadcast", dict(base, a_strides=[0], out_ptr=B)), ("where_raw", "out_ptr is b_ptr, stepped", dict(base, b_strides=[2], out_ptr=C)),
            ("where_raw", "scalar a, no host pointer", dict(base, a_ptr=0, a_strides=None)), ("where_raw", "scalar b, no host pointer", dict(base, b_ptr=0, b_strides=None)),
            ("where_raw", "a span past 2^59", dict(base, x_strides=[1 << 58, 1], a_strides=[4, 1], b_strides=[4, 1], shape=[4, 4]))]

    base = dict(cmp=5, dtype=dt, x_ptr=A, x_strides=[1], y_ptr=0, y_strides=None, rhs=1.0, shape=s8, count_ptr=B)
    out += faults("select_count_raw", base, enums=["cmp"], shape="shape", strides=["x_strides"], ptrs=["x_ptr", "count_ptr", "rhs"], aligned=["x_ptr", "count_ptr"],
                     overlaps=[("count_ptr", w, "x_ptr", 8 * e, w)])
    with_y = dict(base, y_ptr=E, y_strides=[1], rhs=None)
    out += [("select_count_raw", "y: null strides", dict(with_y, y_strides=None)), ("select_count_raw", "y: misaligned", dict(with_y, y_ptr=E + 1)),
            ("select_count_raw", "count_ptr over the front of y", dict(with_y, count_ptr=E)), ("select_count_raw", "count_ptr over the back of y", dict(with_y, count_ptr=E + 8 * e - w)),
            ("select_count_raw", "nonzero needs no rhs; count_ptr over x", dict(base, cmp=0, rhs=None, count_ptr=A + 8)),
            ("select_count_raw", "a transposed x, count_ptr over it", dict(base, shape=[4, 4], x_strides=[1, 4], count_ptr=A + 8)),
            ("select_count_raw", "nothing to count, a null result", dict(base, shape=[0], x_ptr=0, count_ptr=0))]

    base = dict(what=2, cmp=5, dtype=dt, x_ptr=A, x_strides=[1], y_ptr=0, y_strides=None, rhs=1.0, shape=s8, src_ptr=B, src_strides=[1], src_elem_bytes=e, out_ptr=C, capacity=8,
                count_ptr=D)
    out += faults("select_raw", base, enums=["what", "cmp"], shape="shape", strides=["x_strides", "src_strides"], ptrs=["x_ptr", "src_ptr", "out_ptr", "rhs"],
                     aligned=["x_ptr", "src_ptr", "out_ptr", "count_ptr"],
                     overlaps=[("out_ptr", 8 * e, "x_ptr", 8 * e, e), ("out_ptr", 8 * e, "src_ptr", 8 * e, e), ("count_ptr", w, "x_ptr", 8 * e, w), ("count_ptr", w, "src_ptr", 8 * e, w),
                               ("count_ptr", w, "out_ptr", 8 * e, w)],
                     empty=dict(shape=[0], x_ptr=0, src_ptr=0, out_ptr=0, count_ptr=0))
    out += [("select_raw", "src elements of 2 bytes", dict(base, src_elem_bytes=2)), ("select_raw", "a negative capacity", dict(base, capacity=-1)),
            ("select_raw", "a capacity of 2^59", dict(base, capacity=1 << 59)), ("select_raw", "no capacity, no count", dict(base, capacity=0, out_ptr=0, count_ptr=0)),
            ("select_raw", "coords: count_ptr over the second plane", dict(base, what=1, x_strides=[3, 1], shape=[2, 3], src_ptr=0, src_strides=None, capacity=6, count_ptr=C + 88)),
            ("select_raw", "index: out_ptr misaligned for int64", dict(base, what=0, out_ptr=C + 4)),
            # nothing to select from: the result may be null while its capacity is not
            ("select_raw", "no elements, a null result, count_ptr at 8", dict(base, shape=[0], x_ptr=0, src_ptr=0, out_ptr=0, count_ptr=8))]

    # ---- runs
    base = dict(flags=0, dtype=dt, s_ptr=A, n=8, count_ptr=B)
    out += faults("runs_count_raw", base, enums=["flags"], ptrs=["s_ptr", "count_ptr"], aligned=["s_ptr", "count_ptr"], overlaps=[("count_ptr", w, "s_ptr", 8 * e, w)])
    out += [("runs_count_raw", "a negative n", dict(base, n=-1)), ("runs_count_raw", "n of 2^59", dict(base, n=1 << 59)),
            ("runs_count_raw", "nothing to count, a null result", dict(base, n=0, s_ptr=0, count_ptr=0))]

    base = dict(flags=0, dtype=dt, s_ptr=A, n=8, order_ptr=B, values_ptr=C, index_ptr=D, counts_ptr=E, inverse_ptr=F, capacity=8, count_ptr=G)
    out += faults("runs_raw", base, enums=["flags"], ptrs=["s_ptr"], aligned=["s_ptr", "order_ptr", "values_ptr", "index_ptr", "counts_ptr", "inverse_ptr", "count_ptr"],
                     overlaps=[("values_ptr", 8 * e, "s_ptr", 8 * e, e), ("inverse_ptr", 8 * w, "s_ptr", 8 * e, w), ("count_ptr", w, "order_ptr", 8 * w, w),
                               ("index_ptr", 8 * w, "counts_ptr", 8 * w, w), ("values_ptr", 8 * e, "index_ptr", 8 * w, w)],
                     empty=dict(n=0, s_ptr=0, count_ptr=0))
    out += [("runs_raw", "a negative n", dict(base, n=-1)), ("runs_raw", "a negative capacity", dict(base, capacity=-1)),
            ("runs_raw", "no result", dict(base, values_ptr=0, index_ptr=0, counts_ptr=0, inverse_ptr=0)),
            ("runs_raw", "a capacity of 2: the firsts end before counts_ptr", dict(base, capacity=2, index_ptr=E - 2 * w, inverse_ptr=0, s_ptr=0, n=0, count_ptr=0)),
            ("runs_raw", "no capacity, no inverse, no count", dict(base, capacity=0, inverse_ptr=0, count_ptr=0))]
    return out


def plan_cases():
    """The host-only planners: the base call (SMHIP_OK) and the faults their binding methods can express."""
    s35 = [3, 5]
    out = []
    for fn, base, kw in (
            ("reduce_plan", dict(kind=0, dtype=F32, shape=s35, strides=[5, 1], axis=1), dict(enums=["kind"], shape="shape", strides=["strides"])),
            ("scan_plan", dict(kind=0, dtype=F32, shape=s35, strides=[5, 1], axis=1), dict(enums=["kind"], shape="shape", strides=["strides"], axis="axis")),
            ("argreduce_plan", dict(kind=0, dtype=I64, shape=s35, strides=[5, 1], axis=1), dict(enums=["kind"], shape="shape", strides=["strides"], axis="axis")),
            ("sort_plan", dict(dtype=F32, shape=s35, strides=[5, 1], axis=1), dict(shape="shape", strides=["strides"], axis="axis")),
            ("take_plan", dict(dtype=I64, a_strides=[7, 1], a_extent=7, idx_strides=[5, 1], out_shape=s35, axis=1, mode=0),
             dict(enums=["mode"], shape="out_shape", strides=["a_strides", "idx_strides"], axis="axis")),
            ("scatter_plan", dict(dtype=F32, out_shape=s35, axis=1, idx_strides=[4, 1], val_strides=[4, 1], n_entries=4, kind=0, mode=0),
             dict(enums=["kind", "mode"], shape="out_shape", strides=["idx_strides", "val_strides"], axis="axis")),
            ("count_plan", dict(what=2, dtype=F32, shape=[8], strides=[1], bins=4), dict(enums=["what"], shape="shape", strides=["strides"])),
            ("select_plan", dict(what=0, dtype=I64, shape=[8], x_strides=[1], cmp=5), dict(enums=["what", "cmp"], shape="shape", strides=["x_strides"])),
            ("convert_plan", dict(src_dtype=F32, dst_dtype=I64, shape=s35, strides=[5, 1]), dict(dtypes=["src_dtype", "dst_dtype"], shape="shape", strides=["strides"])),
            ("runs_plan", dict(dtype=F32, n=8, outputs=1, flags=0), dict(enums=["flags", "outputs"]))):
        out.append((fn, "well-formed", dict(base)))
        out += [c for c in one_fault(fn, base, plan=True, **kw) if (fn, c[1]) != ("reduce_plan", "ndim=0")]  # the binding's own check comes first there
    out += [("take_plan", "a negative extent of a", dict(dtype=F32, a_strides=[7, 1], a_extent=-1, idx_strides=[5, 1], out_shape=s35, axis=1, mode=0)),
            ("scatter_plan", "a negative number of entries", dict(dtype=F32, out_shape=s35, axis=1, idx_strides=[4, 1], val_strides=[4, 1], n_entries=-1)),
            ("count_plan", "bincount of floats", dict(what=1, dtype=F32, shape=[8], strides=[1], bins=4)),
            ("count_plan", "a negative number of bins", dict(what=2, dtype=F32, shape=[8], strides=[1], bins=-1)),
            ("runs_plan", "a negative n", dict(dtype=F32, n=-1))]
    return out


def cases():
    """Every case, in the table's order: [method, case name, keyword arguments]."""
    return [[fn, name, kw] for fn, name, kw in raw_cases(F32) + raw_cases(I64) + plan_cases()]


def answer(lib, fn, kwargs):
    """(return code, message) of one call; the message of a call that succeeds is ''."""
    import simplemath_amd as sma
    kw = {k: (np.array([v], np.float64) if k in SCALARS and v is not None else v) for k, v in kwargs.items()}
    try:
        rc = getattr(lib, fn)(**kw)
    except sma.SmhipError as err:
        rc = err.code
    if not isinstance(rc, int):  # a planner's answer
        rc = OK
    return rc, lib.c.smhip_last_error().decode() if rc != OK else ""


def main():
    sys.path.insert(0, ROOT)
    import simplemath_amd as sma
    lib = sma.load()
    if lib.device_count():
        raise SystemExit("this machine has a device: a call that got past the checks would launch on made-up pointers")
    rows = []
    for fn, name, kw in cases():
        rc, msg = answer(lib, fn, kw)
        if rc not in (OK, INVALID, UNSUPPORTED):
            raise SystemExit("%s, %r: got past the checks (%d: %s) -- not a refusal, take it out of the list" % (fn, name, rc, msg))
        rows.append([fn, name, kw, rc, msg])
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print("%d rows -> %s" % (len(rows), TABLE))


if __name__ == "__main__":
    main()
