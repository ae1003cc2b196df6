"""Soak of the axis families over random views, steered by what the host planners answer.

usage: python tests/fuzz_axis.py [cases] [seed] [trace file] [--plan-only] [--keep-going]   -- prints the first mismatch and exits 1;
otherwise "ok: N cases", the coverage tables and "skipped 0".  --plan-only draws the same cases and asks the planners, without a
device.  --keep-going prints every mismatch instead of the first (it still stops at the first error of the HIP runtime).

A case is one call of one family -- reduce, scan, argreduce, sort / argsort, topk, softmax / log_softmax / logsumexp, take_along_axis /
take, put_along_axis / scatter_add, searchsorted / bincount, select / flatnonzero, unique, astype -- on a random view: rank 1 to 6,
slices with steps, a permutation, size-1 axes, a stride-0 axis, and a first element that is off a 16-byte boundary in about half of
the cases.  Every fifth case is a pipeline (PROGRAMS): 2 to 4 dependent operators of the axis families, fed by and feeding tracked
operators (astype, unary, where, elementwise) and a recorded tiny elementwise operator, all issued without a host wait.

Steering.  Each family has a `*_plan` method that touches no device, and a case's coverage row is (family, route, flags) as that
planner answers it.  The families take turns, each in proportion to its rows; a family's cases take its rows in turn, and a case's
view is drawn again (from random shapes and from the shapes the planner tests name) until the planner answers the wanted row.  The
view traits (TRAITS) take turns in the same way and are forced into the draw.  So the tables depend on (cases, seed) alone, and
tests/test_fuzz_axis_host.py holds them to at least 3 per row without a device.

Nothing is compared here by a rule of this file: every check is the comparator of the family's own tests/test_*_gpu.py (which states
the contract of include/smhip.h against numpy in higher precision), on values from those files' generators."""
import contextlib
import io
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from numpy.lib.stride_tricks import as_strided  # noqa: E402

import simplemath_amd as sma  # noqa: E402
from tests import test_argreduce_gpu as t_arg  # noqa: E402
from tests import test_astype_gpu as t_cvt  # noqa: E402
from tests import test_axis_reduce_gpu as t_red  # noqa: E402
from tests import test_count_gpu as t_cnt  # noqa: E402
from tests import test_scan_gpu as t_scan  # noqa: E402
from tests import test_scatter_gpu as t_sct  # noqa: E402
from tests import test_select_gpu as t_sel  # noqa: E402
from tests import test_softmax_gpu as t_sm  # noqa: E402
from tests import test_sort_gpu as t_sort  # noqa: E402
from tests import test_take_gpu as t_take  # noqa: E402
from tests import test_topk_gpu as t_topk  # noqa: E402
from tests import test_unary_gpu as t_un  # noqa: E402
from tests import test_unique_gpu as t_unq  # noqa: E402
from tests import util  # noqa: E402

SMOKE_CASES, SMOKE_SEED = 700, 7      # what tests/test_fuzz_axis_host.py and tests/test_fuzz_axis_gpu.py run
FLOATS = (np.float32, np.float64)
INTS = (np.int32, np.int64)
ALL = FLOATS + INTS
MAX_ELEMS = 1 << 20                    # no operand is larger
USUAL_ELEMS = 1 << 17                  # most cases stay at or below this
TRAITS = ("misaligned first element", "stride-0 axis", "permuted", "stepped", "size-1 axis", "rank >= 5")
GRID_CAPS = ("REDUCE", "SCAN", "ARGREDUCE", "SORT", "TOPK", "SOFTMAX", "TAKE", "SCATTER", "COUNT", "SELECT")

# The rows a planner can answer with operands of at most 2^20 elements.  (The 2^31 clamps, "at most 256 chunks" and "more than 4096
# chunks" need more: tests/test_past_2p31_gpu.py and the plan table own them.)  A row a case reaches that is not listed is an error.
ROWS = {
    "reduce": ["NONE", "FILL", "GATHER", "ROW short g=4", "ROW short g=16", "ROW short g=64", "ROW long", "ROW long|SPLIT", "COLUMN", "COLUMN|SPLIT",
               "CHANNEL", "CHANNEL|SPLIT", "ROW short g=4|COPY", "ROW short g=16|COPY", "ROW short g=64|COPY", "ROW long|COPY", "ROW long|SPLIT|COPY",
               "COLUMN|COPY", "COLUMN|SPLIT|COPY", "CHANNEL|COPY", "CHANNEL|SPLIT|COPY", "PASSES 2 groups", "PASSES 2 groups|COPY", "PASSES 3 groups",
               "PASSES 3 groups|COPY"],
    "scan": ["NONE", "COPYONLY", "ROW short g=4", "ROW short g=16", "ROW short g=64", "ROW long", "ROW long|SPLIT", "COLUMN", "COLUMN|SPLIT",
             "ROW short g=4|COPY", "ROW short g=16|COPY", "ROW short g=64|COPY", "ROW long|COPY", "ROW long|SPLIT|COPY", "COLUMN|COPY", "COLUMN|SPLIT|COPY"],
    "arg": ["NONE", "ROW short g=4", "ROW short g=16", "ROW short g=64", "ROW long", "ROW long|SPLIT", "COLUMN", "COLUMN|SPLIT",
            "ROW short g=4|COPY", "ROW short g=16|COPY", "ROW short g=64|COPY", "ROW long|COPY", "ROW long|SPLIT|COPY", "COLUMN|COPY", "COLUMN|SPLIT|COPY"],
    "sort": ["NONE", "COPYONLY", "ROW", "ROW|MERGE", "ROW|COPY", "ROW|MERGE|COPY"],
    "topk": ["NONE", "COPYONLY", "ROW ranked", "ROW", "ROW|TILED", "SORT", "ROW ranked|COPY", "ROW|COPY", "ROW|TILED|COPY", "SORT|COPY"],
    "softmax": ["NONE", "FILL", "ROW segment g=4", "ROW segment g=16", "ROW segment g=64", "ROW wave", "ROW workgroup", "ROW|SPLIT", "COLUMN",
                "COLUMN|SPLIT", "ROW segment g=4|COPY", "ROW segment g=16|COPY", "ROW segment g=64|COPY", "ROW wave|COPY", "ROW workgroup|COPY",
                "ROW|SPLIT|COPY", "COLUMN|COPY", "COLUMN|SPLIT|COPY"],
    "take": ["NONE", "LINE", "ROWS", "DIRECT", "LINE|COPY", "ROWS|COPY", "DIRECT|COPY"],
    "scatter": ["NONE", "DIRECT", "ROWS", "SORTED", "SORTED_ROWS", "DIRECT|COPY", "ROWS|COPY", "SORTED|COPY", "SORTED_ROWS|COPY"],
    "count": ["searchsorted NONE", "searchsorted LDS", "searchsorted GLOBAL", "searchsorted LDS|COPY", "searchsorted GLOBAL|COPY",
              "bincount NONE", "bincount LDS", "bincount GLOBAL", "bincount LDS|COPY", "bincount GLOBAL|COPY"],
    "select": ["NONE", "ONE", "TILES", "ONE|COPY", "TILES|COPY"],
    "runs": ["NONE", "ONE", "TILES"],
    "convert": ["NONE", "DENSE", "ROWS", "STAGED", "COPY"],
}
FAMILIES = tuple(ROWS)
MIN_TURNS = 12   # a family's turns per round: its rows, but at least this many (the view traits need them)


def prod(seq):
    out = 1
    for n in seq:
        out *= int(n)
    return out


def pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def name_of(dt):
    return np.dtype(dt).name


# ====================================================================================================== views
class View:
    """A view of a 1-D buffer: shape, strides and offset in elements; `wshape` is the shape with the stride-0 axis collapsed to 1 (the
    elements that exist).  Stands in for a DeviceArray where only shape and strides are asked (the planners, call_args)."""

    def __init__(self, shape, strides, offset, nbuf, z, traits, dtype):
        self.shape, self.strides, self.offset, self.nbuf, self.z, self.traits = tuple(shape), tuple(strides), offset, nbuf, z, traits
        self.dtype = np.dtype(dtype)
        self.wshape = tuple(1 if d == z else n for d, n in enumerate(shape))
        self.ndim, self.size = len(shape), prod(shape)

    def host(self, vals, rng):
        """-> (the buffer, the view of it as a read-only numpy array) with `vals` (of wshape) as the view's elements and other values
        of the same kind everywhere else."""
        dt = self.dtype
        assert self.offset + sum((n - 1) * s for n, s in zip(self.shape, self.strides) if n > 0) < self.nbuf and min(self.strides) >= 0, self  # inside the buffer
        if dt.kind == "f":
            buf = (rng.standard_normal(self.nbuf) * 100).astype(dt)
        else:
            buf = rng.integers(-1000, 1000, size=self.nbuf).astype(dt)
        sb = [s * dt.itemsize for s in self.strides]
        if prod(self.wshape):
            as_strided(buf[self.offset:], shape=self.wshape, strides=sb)[...] = np.asarray(vals, dtype=dt).reshape(self.wshape)
        return buf, as_strided(buf[self.offset:], shape=self.shape, strides=sb, writeable=False)

    def __repr__(self):
        return f"{self.dtype.name}{list(self.shape)} strides {list(self.strides)} offset {self.offset}"


def draw_view(rng, shape, dtype, z=None, force=None, plain=False):
    """A random view geometry for `shape`: axes in a random memory order, steps of 1 to 3, margins before and after, and a lead that
    puts the first element on or off a 16-byte boundary.  `z` names the stride-0 axis; `force` a trait the view must have; `plain`
    gives a dense row-major array (only the lead is drawn), which the in-place forms need."""
    nd, item = len(shape), np.dtype(dtype).itemsize
    W, size = 16 // item, prod(shape)
    live = [d for d in range(nd) if shape[d] > 1 and d != z]
    rich = size <= USUAL_ELEMS and not plain
    order = list(range(nd))
    if not plain and len(live) >= 2 and (force == "permuted" or rng.random() < 0.35):
        while [d for d in order if d in live] == live:
            order = [int(v) for v in rng.permutation(nd)]
    step, lo, hi = [1] * nd, [0] * nd, [0] * nd
    if not plain:
        for d in range(nd):
            if not rich and d != order[-1]:
                continue
            if rich and rng.random() < 0.25:
                step[d] = int(pick(rng, [2, 3]))
            if rng.random() < 0.4:
                lo[d] = int(rng.integers(0, 3))
            if rng.random() < 0.4:
                hi[d] = int(rng.integers(0, 3))
        if force == "stepped" and live and not any(step[d] > 1 for d in live):
            step[min(live, key=lambda d: shape[d])] = 2
    ext = [lo[d] + (max(1 if d == z else shape[d], 1) - 1) * step[d] + 1 + hi[d] for d in range(nd)]
    mst, acc = [0] * nd, 1
    for d in reversed(order):
        mst[d] = acc
        acc *= ext[d]
    strides = [0 if d == z else mst[d] * step[d] for d in range(nd)]
    voff = sum(lo[d] * mst[d] for d in range(nd))
    misaligned = True if force == "misaligned first element" else bool(rng.random() < 0.5)
    lead = int(pick(rng, [o for o in range(W) if ((o + voff) % W != 0) == misaligned]))
    traits = set()
    if size and misaligned:
        traits.add(TRAITS[0])
    if z is not None and shape[z] > 1:
        traits.add(TRAITS[1])
    if [d for d in order if d in live] != live:
        traits.add(TRAITS[2])
    if any(step[d] > 1 for d in live):
        traits.add(TRAITS[3])
    if any(n == 1 for n in shape):
        traits.add(TRAITS[4])
    if nd >= 5:
        traits.add(TRAITS[5])
    return View(shape, strides, lead + voff, lead + acc + int(rng.integers(0, 3)), z, traits, dtype)


EXTENTS = (2, 3, 4, 5, 7, 8, 13, 16, 17, 33, 61, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1025, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 9001,
           16385, 40001, 70001, 131073, 262149, 524291)


def draw_shape(rng, limit, force=None, zero=0.03):
    """A shape of rank 1 to 6 with at most `limit` elements: small extents (1 among them) and up to two from EXTENTS."""
    nd = int(pick(rng, [1, 2, 2, 3, 3, 4, 5, 6]))
    if force == "rank >= 5":
        nd = int(pick(rng, [5, 6]))
    elif force in ("permuted", "size-1 axis"):
        nd = max(nd, 2)
    shape = [int(pick(rng, [1, 2, 3, 4, 5, 7, 9] if nd <= 4 else [1, 1, 2, 2, 3, 5])) for _ in range(nd)]
    for d in rng.permutation(nd)[:int(pick(rng, [0, 1, 1, 1, 2, 2]))]:
        shape[d] = 1
        fit = [e for e in EXTENTS if e * prod(shape) <= limit]
        shape[d] = int(pick(rng, fit)) if fit else 1
    while prod(shape) > limit:
        d = int(np.argmax(shape))
        shape[d] = max(1, shape[d] // 2)
    if force == "size-1 axis" and 1 not in shape:
        shape[int(np.argmin(shape))] = 1
    if rng.random() < zero:
        shape[int(rng.integers(0, nd))] = 0
    return shape


def decorate(rng, core, axes, force=None):
    """A hinted core shape with size-1 axes put in (up to rank 6): -> (shape, where the core's `axes` are now)."""
    want = 0
    if force == "rank >= 5":
        want = int(pick(rng, [5, 6])) - len(core)
    elif force == "size-1 axis" or rng.random() < 0.3:
        want = int(rng.integers(1, 3))
    want = max(0, min(want, 6 - len(core)))
    slots = sorted(int(v) for v in rng.integers(0, len(core) + 1, size=want))
    shape, where = [], {}
    for d in range(len(core) + 1):
        shape += [1] * slots.count(d)
        if d < len(core):
            where[d] = len(shape)
            shape.append(int(core[d]))
    return shape, [where[a] for a in axes]


def pick_z(rng, shape, force, p=0.12):
    """The stride-0 axis of a view: one of extent > 1, or None."""
    live = [d for d in range(len(shape)) if shape[d] > 1]
    if live and (force == "stride-0 axis" or rng.random() < p):
        return int(pick(rng, live))
    return None


def shape_and_axis(rng, limit, force, hints):
    """-> (shape, axis): a random shape and axis, or (half of the time, where the family has hints) a hinted core decorated."""
    if hints and rng.random() < 0.5:
        core, axis = hints[int(rng.integers(0, len(hints)))]
        if prod(core) <= limit:
            shape, (axis,) = decorate(rng, core, [axis], force)
            return shape, axis
    shape = draw_shape(rng, limit, force)
    return shape, int(rng.integers(0, len(shape)))


def seg(R, dt):
    """axis_plan.h's segment_lanes(row_loads(R, W)): the lanes of a short row, 0 for a longer one."""
    W = 16 // np.dtype(dt).itemsize
    loads = R // W + R % W
    return 4 if loads <= 4 else 16 if loads <= 16 else 64 if loads <= 64 else 0


def flagged(name, word, flags):
    return name + "".join("|" + text for bit, text in flags if word & bit)


# ====================================================================================================== the families
# cand_*(rng, lib, limit, force) -> a case without values (a dict: fam, row, what, views, ...), or None where the draw is one the
# contract refuses.  vals_*(case, rng) -> the views' values.  run_*(lib, case, ops) checks it on the device; ops[k] = (host view,
# device view) of case["views"][k].
def row_kernel(names, word, ori_r, dt, flags, short=True):
    name = names[word & 0xff]
    if name == "ROW" and short:
        g = seg(ori_r, dt)
        name = f"ROW short g={g}" if g else "ROW long"
    return flagged(name, word, flags)


def cand_reduce(rng, lib, limit, force):
    kind = str(pick(rng, t_red.KINDS))
    dt = FLOATS[int(rng.integers(0, 2))] if kind == "mean" else ALL[int(rng.integers(0, 4))]
    hints = [((64, 224, 3), (0, 1)), ((4, 4096, 3), (1,)), ((1000, 4, 3), (1,)), ((1000, 300), (0,)), ((4, 70001), (1,)), ((262149, 3), (0,)),
             ((5, 60, 7), (0, 2)), ((3, 4, 5, 6, 7), (0, 2, 4)), ((2, 3, 4, 5, 3, 2), (1, 3, 5)), ((300, 1, 40), (1,)), ((2, 131073), (1,)), ((7, 1024, 3), (1,)), ((1024, 5), (0,)), ((3, 4, 5, 6, 7), (1, 3)), ((11, 4097), (1,))]
    if rng.random() < 0.5:
        core, axes = hints[int(rng.integers(0, len(hints)))]
        if prod(core) > limit:
            return None
        shape, axes = decorate(rng, core, axes, force)
    else:
        shape = draw_shape(rng, limit, force)
        axes = sorted(int(v) for v in rng.choice(len(shape), size=min(len(shape), int(pick(rng, [1, 1, 2, 3]))), replace=False))
    nr, nout = prod(shape[d] for d in axes), prod(n for d, n in enumerate(shape) if d not in axes)
    if nr == 0:
        kind = "sum"   # mean / max / min over an empty extent is refused (and numpy raises)
    v = draw_view(rng, shape, dt, pick_z(rng, shape, force), force, plain=bool(rng.random() < 0.2))
    word, _, ori = lib.reduce_plan(kind, dt, list(shape), list(v.strides), tuple(axes))
    if word & sma.ROUTE_PASSES:
        live = [d in axes for d in range(len(shape)) if shape[d] > 1]
        groups = sum(1 for k, r in enumerate(live) if r and (k == 0 or not live[k - 1]))
        row = flagged(f"PASSES {groups} groups", word, [(sma.ROUTE_COPY, "COPY")])
    else:
        row = row_kernel(["NONE", "ROW", "COLUMN", "CHANNEL", "FILL", "GATHER"], word, ori[1], dt, [(sma.ROUTE_SPLIT, "SPLIT"), (sma.ROUTE_COPY, "COPY")])
    return dict(fam="reduce", row=row, views=[v], kind=kind, axes=tuple(axes), keepdims=bool(rng.random() < 0.5), what=f"{kind} axes {tuple(axes)}")


def vals_reduce(c, rng):
    return [t_red.sample(c["views"][0].wshape, c["views"][0].dtype.type, int(rng.integers(1 << 30)))]


def run_reduce(lib, c, ops):
    x, dx = ops[0]
    t_red.check(c["kind"], x, c["axes"], lib.reduce(c["kind"], dx, c["axes"], keepdims=c["keepdims"]).numpy(), keepdims=c["keepdims"])


SCAN_HINTS = [((4, 8192), 1), ((1, 262149), 1), ((3, 70001), 1), ((70001, 8), 0), ((9001, 5, 7), 0), ((300, 4099), 0), ((500, 1, 33), 1), ((1000, 13), 1),
              ((300, 61), 1), ((70, 255), 1), ((11, 9001), 1), ((6, 40001), 1), ((1, 512), 0), ((512, 1), 1)]


def cand_scan(rng, lib, limit, force):
    kind, dt = str(pick(rng, t_scan.KINDS)), ALL[int(rng.integers(0, 4))]
    shape, axis = shape_and_axis(rng, limit, force, SCAN_HINTS)
    inplace = force in (None, TRAITS[0], TRAITS[4], TRAITS[5]) and prod(shape) > 0 and rng.random() < 0.15
    v = draw_view(rng, shape, dt, None if inplace else pick_z(rng, shape, force), force, plain=inplace)
    word, _, ori, _ = lib.scan_plan(kind, dt, list(shape), list(v.strides), axis)
    row = row_kernel(["NONE", "COPYONLY", "ROW", "COLUMN"], word, ori[1], dt, [(sma.SCAN_SPLIT, "SPLIT"), (sma.SCAN_COPY, "COPY")])
    R = shape[axis]
    rounded = np.dtype(dt).kind == "f" and kind in ("cumsum", "cumprod") and prod(shape) > 0 and (kind == "cumsum" or R <= 400) and \
        (rng.random() < 0.4 or (kind == "cumprod" and v.z == axis))
    if np.dtype(dt).kind == "f" and kind == "cumprod" and v.z == axis and not rounded:
        return None   # a product of one repeated factor of the exact kind leaves the range
    return dict(fam="scan", row=row, views=[v], kind=kind, axis=axis, inplace=inplace, rounded=rounded,
                what=f"{kind} axis {axis}{' in place' if inplace else ''}{' rounded data' if rounded else ''}")


def vals_scan(c, rng):
    v, kind = c["views"][0], c["kind"]
    dt = v.dtype.type
    if not c["rounded"]:
        return [t_scan.exact_input(kind, v.wshape, dt, c["axis"], int(rng.integers(1 << 30)))]
    if kind == "cumsum":   # test_scan_gpu.test_rounded_data_within_the_contract_bound's two kinds of data
        return [(rng.standard_normal(v.wshape) * 10.0).astype(dt)]
    return [(rng.uniform(0.5, 2.0, size=v.wshape) * rng.choice(np.array([-1.0, 1.0]), size=v.wshape)).astype(dt)]


def run_scan(lib, c, ops):
    x, dx = ops[0]
    kind, axis = c["kind"], c["axis"]
    host = np.array(x)   # (an in-place call overwrites what x views)
    got = lib.scan(kind, dx, axis, out=dx if c["inplace"] else None)
    assert not c["inplace"] or got is dx
    got = got.numpy()
    assert got.shape == host.shape
    if c["rounded"]:
        t_scan.check_rounded(kind, host, axis, got)
    else:
        assert np.array_equal(got, t_scan.expected(kind, host, axis)), (kind, host.dtype, host.shape, axis)


ARG_HINTS = [((4, 70001), 1), ((1, 262149), 1), ((70001, 3), 0), ((9001, 5, 7), 0), ((300, 4099), 0), ((1000, 13), 1), ((300, 61), 1), ((70, 255), 1),
             ((11, 9001), 1), ((6, 40001), 1)]


def cand_arg(rng, lib, limit, force):
    kind, dt = str(pick(rng, t_arg.KINDS)), ALL[int(rng.integers(0, 4))]
    shape, axis = shape_and_axis(rng, limit, force, ARG_HINTS)
    if shape[axis] == 0:
        return None   # argmax over an empty axis is refused
    v = draw_view(rng, shape, dt, pick_z(rng, shape, force), force)
    word, _, ori, _ = lib.argreduce_plan(kind, dt, list(shape), list(v.strides), axis)
    row = row_kernel(["NONE", "ROW", "COLUMN"], word, ori[1], dt, [(sma.ARG_SPLIT, "SPLIT"), (sma.ARG_COPY, "COPY")])
    return dict(fam="arg", row=row, views=[v], kind=kind, axis=axis, keepdims=bool(rng.random() < 0.5), values=bool(rng.random() < 0.5),
                data="ties" if rng.random() < 0.4 else "continuous", what=f"{kind} axis {axis}")


def vals_arg(c, rng):
    v = c["views"][0]
    return [getattr(t_arg, c["data"])(v.wshape, v.dtype.type, int(rng.integers(1 << 30)))]


def run_arg(lib, c, ops):
    x, dx = ops[0]
    if c["values"]:
        vals, idx = lib.argreduce(c["kind"], dx, c["axis"], keepdims=c["keepdims"], values=True)
        t_arg.check(c["kind"], x, c["axis"], idx.numpy(), vals.numpy(), c["keepdims"])
    else:
        t_arg.check(c["kind"], x, c["axis"], lib.argreduce(c["kind"], dx, c["axis"], keepdims=c["keepdims"]).numpy(), None, c["keepdims"])


SORT_HINTS = [((7, 4097), 1), ((3, 8193), 1), ((1, 70001), 1), ((4097, 5), 0), ((33, 1, 7), 1), ((300, 257), 1), ((5, 4096), 1), ((2, 20001), 1)]


def sort_data(rng):
    return str(pick(rng, ["continuous", "continuous", "ties", "ties", "specials"]))


def cand_sort(rng, lib, limit, force):
    dt = ALL[int(rng.integers(0, 4))]
    shape, axis = shape_and_axis(rng, min(limit, 1 << 18), force, SORT_HINTS)
    v = draw_view(rng, shape, dt, pick_z(rng, shape, force), force)
    desc = bool(rng.random() < 0.5)
    word, _, _, _ = lib.sort_plan(dt, list(shape), list(v.strides), axis, desc)
    row = flagged(["NONE", "COPYONLY", "ROW"][word & 0xff], word, [(sma.SORT_MERGE, "MERGE"), (sma.SORT_COPY, "COPY")])
    mode = str(pick(rng, t_sort.MODES))
    return dict(fam="sort", row=row, views=[v], axis=axis, desc=desc, mode=mode, data=sort_data(rng), what=f"sort axis {axis} descending {desc} {mode}")


def vals_sorted_kind(c, rng):
    v = c["views"][0]
    return [getattr(t_sort, c["data"] if prod(v.wshape) else "continuous")(v.wshape, v.dtype.type, int(rng.integers(1 << 30)))]


def run_sort(lib, c, ops):
    x, dx = ops[0]
    t_sort.check(lib, x, dx, c["axis"], c["mode"], orders=(c["desc"],))


TOPK_HINTS = [((7, 4097), 1), ((3, 8193), 1), ((1, 70001), 1), ((4097, 5), 0), ((33, 1, 7), 1), ((300, 257), 1), ((500, 128), 1), ((500, 129), 1),
              ((40, 2049), 1), ((2, 40001), 1)]


def cand_topk(rng, lib, limit, force):
    dt = ALL[int(rng.integers(0, 4))]
    shape, axis = shape_and_axis(rng, min(limit, 1 << 18), force, TOPK_HINTS)
    v = draw_view(rng, shape, dt, pick_z(rng, shape, force), force)
    R = shape[axis]
    kmax = lib.topk_plan(dt, [1 << 20], [1], 0, 1)[3][1]
    ks = sorted({k for k in (1, 2, 5, 63, 64, 65, R // 2, R // 2 + 1, kmax - 1, kmax, kmax + 1, R - 1, R) if 0 < k <= R}) or [0]
    k = 0 if rng.random() < 0.04 else int(pick(rng, ks))
    largest = bool(rng.random() < 0.5)
    word, _, _, _ = lib.topk_plan(dt, list(shape), list(v.strides), axis, k, largest)
    name = ["NONE", "COPYONLY", "ROW", "SORT"][word & 0xff]
    if name == "ROW" and R <= sma.TOPK_RANKED:
        name = "ROW ranked"
    row = flagged(name, word, [(sma.TOPK_TILED, "TILED"), (sma.TOPK_COPY, "COPY")])
    mode = str(pick(rng, t_topk.MODES))
    return dict(fam="topk", row=row, views=[v], axis=axis, k=k, largest=largest, mode=mode, data=sort_data(rng), what=f"topk k {k} axis {axis} largest {largest} {mode}")


def run_topk(lib, c, ops):
    x, dx = ops[0]
    t_topk.check(lib, x, dx, [c["k"]], c["axis"], c["mode"], orders=(c["largest"],))


SOFTMAX_HINTS = [((5, 8193), 1), ((3, 4097), 1), ((2, 70001), 1), ((70001, 3), 0), ((300, 4099), 0), ((70, 50), 0), ((9001, 5, 7), 0), ((1000, 13), 1),
                 ((300, 61), 1), ((70, 255), 1), ((40, 1000), 1), ((9, 8192), 1), ((9, 4096), 1), ((9, 2049), 1), ((3, 0), 1)]


def cand_softmax(rng, lib, limit, force):
    kind, dt = str(pick(rng, t_sm.KINDS)), FLOATS[int(rng.integers(0, 2))]
    shape, axis = shape_and_axis(rng, limit, force, SOFTMAX_HINTS)
    inplace = kind != "logsumexp" and force in (None, TRAITS[0], TRAITS[4], TRAITS[5]) and prod(shape) > 0 and rng.random() < 0.15
    v = draw_view(rng, shape, dt, None if inplace else pick_z(rng, shape, force), force, plain=inplace)
    word, _, ori, _ = lib.softmax_plan(kind, dt, list(shape), list(v.strides), axis)
    name = ["NONE", "ROW", "COLUMN", "FILL"][word & 0xff]
    if name == "ROW" and not word & sma.SOFTMAX_SPLIT:
        g, R = seg(ori[1], dt), ori[1]
        name = f"ROW segment g={g}" if g else "ROW wave" if R <= 64 * 4 * (16 // np.dtype(dt).itemsize) else "ROW workgroup"
    row = flagged(name, word, [(sma.SOFTMAX_SPLIT, "SPLIT"), (sma.SOFTMAX_COPY, "COPY")])
    return dict(fam="softmax", row=row, views=[v], kind=kind, axis=axis, inplace=inplace, keepdims=bool(kind == "logsumexp" and rng.random() < 0.5),
                scale=float(pick(rng, t_sm.SCALES[dt])), what=f"{kind} axis {axis}{' in place' if inplace else ''}")


def vals_softmax(c, rng):
    v = c["views"][0]
    return [t_sm.draws(v.wshape, v.dtype.type, c["scale"], int(rng.integers(1 << 30)))]


def run_softmax(lib, c, ops):
    x, dx = ops[0]
    kind, axis = c["kind"], c["axis"]
    host = np.array(x)
    if kind == "logsumexp":
        got = lib.logsumexp(dx, axis, keepdims=c["keepdims"])
    else:
        got = getattr(lib, kind)(dx, axis, out=dx if c["inplace"] else None)
        assert not c["inplace"] or got is dx
    got = got.numpy()
    if host.shape[axis] == 0 or host.size == 0:   # test_softmax_gpu.test_empty_extents: nothing written, or every output -inf
        if kind == "logsumexp":
            want = np.full(host.shape[:axis] + ((1,) if c["keepdims"] else ()) + host.shape[axis + 1:] or (1,), -np.inf, host.dtype)
            assert got.shape == want.shape and got.tobytes() == want.tobytes()
        else:
            assert got.shape == host.shape
        return
    t_sm.Reference(host, axis).check(kind, got, c["what"])


def index_view(rng, shape, force, z=None):
    return draw_view(rng, shape, np.int64, z, force if force in (TRAITS[0], TRAITS[2], TRAITS[3]) else None, plain=bool(rng.random() < 0.3))


def cand_take(rng, lib, limit, force):
    dt = ALL[int(rng.integers(0, 4))]
    hints = [((1000, 37), 1), ((33, 300), 1), ((7, 4097), 1), ((50, 64), 0), ((300, 257), 0), ((2, 500), 1), ((1, 3), 1), ((5, 9001), 1), ((40001, 3), 0)]
    shape, axis = shape_and_axis(rng, limit // 4, force, hints)
    shape = [max(n, 1) for n in shape]
    R, nd = shape[axis], len(shape)
    mode = str(pick(rng, t_take.MODES))
    room = max(1, (limit // 2) // max(1, prod(shape) // R))
    J = 0 if rng.random() < 0.04 else int(pick(rng, [j for j in (1, 2, R // 2 + 1, R, R + 3, 3 * R + 1, 1000, 70001) if j <= room] or [1]))
    va = draw_view(rng, shape, dt, pick_z(rng, shape, force), force)
    if rng.random() < 0.7:
        form = "take_along_axis"
        ishape = [J if d == axis else (1 if rng.random() < 0.15 else n) for d, n in enumerate(shape)]
        vi = index_view(rng, ishape, force, pick_z(rng, ishape, None, 0.1))
        sa, _, si, oshape = t_take.call_args(va, vi, axis)
    else:
        form = "take"
        vi = index_view(rng, [J], force)
        oshape = [J if d == axis else n for d, n in enumerate(shape)]
        sa, si = list(va.strides), [vi.strides[0] if d == axis else 0 for d in range(nd)]
    word = lib.take_plan(dt, sa, R, si, oshape, axis, mode)[0]
    row = flagged(["NONE", "LINE", "ROWS", "DIRECT"][word & 0xff], word, [(sma.TAKE_COPY, "COPY")])
    return dict(fam="take", row=row, views=[va, vi], form=form, axis=axis, mode=mode, data="specials" if rng.random() < 0.3 else "distinct",
                index=str(pick(rng, t_take.KINDS)), what=f"{form} axis {axis} mode {mode}")


def vals_take(c, rng):
    va, vi = c["views"]
    seed = int(rng.integers(1 << 20))
    a = t_take.specials(va.wshape, va.dtype.type, seed) if c["data"] == "specials" else t_take.distinct(va.wshape, va.dtype.type, seed)
    if c["form"] == "take":
        return [a, t_take.indices(c["index"], vi.wshape, 0, va.shape[c["axis"]], seed)]
    return [a, t_take.indices(c["index"], vi.wshape, c["axis"], va.shape[c["axis"]], seed)]


def run_take(lib, c, ops):
    (a, da), (idx, di) = ops
    if idx.size == 0:   # test_take_gpu.test_empty_results: nothing to gather is a no-op (the flag word is not touched), the shape is numpy's
        fn = lib.take_along_axis if c["form"] == "take_along_axis" else lib.take
        want = (np.take_along_axis if c["form"] == "take_along_axis" else np.take)(a, np.zeros(idx.shape, np.int64), c["axis"])
        got = fn(da, di, c["axis"], mode=c["mode"])
        assert got.shape == want.shape and got.dtype == a.dtype
        return
    if c["form"] == "take_along_axis":
        t_take.check(lib, a, da, idx, di, c["axis"], modes=(c["mode"],))
        return
    t_take.take_case(lib, a, da, np.ascontiguousarray(idx), c["axis"], modes=(c["mode"],))   # (take_case uploads the ids itself: a dense array)
    pos, bad = t_take.normalise(np.ascontiguousarray(idx), a.shape[c["axis"]], c["mode"])
    if not bad:   # and the view of them through the public form
        assert lib.take(da, di, c["axis"], mode=c["mode"]).numpy().tobytes() == np.ascontiguousarray(np.take(a, pos, c["axis"])).tobytes(), "take of a view of ids"


def cand_scatter(rng, lib, limit, force):
    dt = ALL[int(rng.integers(0, 4))]
    kind = int(rng.integers(0, 2))
    hints = [((1000, 37), 1), ((33, 300), 1), ((7, 4097), 1), ((50, 64), 0), ((300, 257), 0), ((1, 70001), 1), ((40001, 3), 0), ((5, 9001), 1)]
    shape, axis = shape_and_axis(rng, limit // 4, force if force in (TRAITS[4], TRAITS[5]) else None, hints)
    shape = [max(n, 1) for n in shape]
    R = shape[axis]
    unique = bool(rng.random() < 0.4)
    mode = str(pick(rng, t_sct.MODES))
    room = max(1, (limit // 4) // max(1, prod(shape) // R))
    room = min(room, R) if unique else room if kind else min(room, 4097)   # (the reference of a put walks the entries one by one)
    J = 0 if rng.random() < 0.04 else int(pick(rng, [j for j in (1, 2, R // 2 + 1, R, R + 3, 3 * R + 1, 1000, 4097, 70001) if j <= room] or [1]))
    walk = [J if d == axis else n for d, n in enumerate(shape)]
    ishape = [n if d == axis or rng.random() > 0.15 else 1 for d, n in enumerate(walk)]
    vshape = [1 if rng.random() < 0.2 else n for n in walk]
    vi = index_view(rng, ishape, force, None if unique else pick_z(rng, ishape, None, 0.1))
    vv = draw_view(rng, vshape, dt, pick_z(rng, vshape, force), force)
    trouble = not unique and rng.random() < 0.1
    word = lib.scatter_plan(dt, shape, axis, t_sct.strides_against(walk, vi, vi), t_sct.strides_against(walk, vv, vv), J, unique=unique, kind=kind, mode=mode)[0]
    row = flagged(["NONE", "DIRECT", "ROWS", "SORTED", "SORTED_ROWS"][word & 0xff], word, [(sma.SCATTER_COPY, "COPY")])
    return dict(fam="scatter", row=row, views=[vv, vi], shape=tuple(shape), dt=dt, kind=kind, axis=axis, mode=mode, unique=unique, trouble=trouble,
                index=str(pick(rng, t_sct.KINDS)), target=int(rng.integers(0, 3)), misalign=int(rng.integers(0, 2)),
                what=f"{'scatter_add' if kind else 'put_along_axis'} into {name_of(dt)}{list(shape)} axis {axis} mode {mode} unique {unique}")


def vals_scatter(c, rng):
    vv, vi = c["views"]
    seed, R, axis = int(rng.integers(1 << 20)), c["shape"][c["axis"]], c["axis"]
    c["a"] = t_sct.operand(c["target"], c["shape"], c["dt"], seed)
    if c["unique"]:
        full = list(vi.wshape)
        full[axis] = R
        idx = np.take(t_sct.permutations(tuple(full), axis, seed), range(vi.wshape[axis]), axis)
    elif c["trouble"]:
        idx = t_sct.trouble_indices(vi.wshape, R, seed)
    else:
        idx = t_sct.indices(c["index"], vi.wshape, axis, R, seed)
    return [t_sct.general(vv.wshape, c["dt"], seed + 1), idx]


def run_scatter(lib, c, ops):
    (values, dv), (idx, di) = ops
    if idx.size == 0:   # test_scatter_gpu.test_empty_cases: no entries is a no-op (the flag word is not touched), the target keeps its bytes
        d = lib.to_device(c["a"])
        fn = lib.scatter_add if c["kind"] else lib.put_along_axis
        assert fn(d, di, dv, c["axis"], mode=c["mode"], unique=c["unique"]) is d and d.numpy().tobytes() == c["a"].tobytes()
        return
    t_sct.check(lib, c["kind"], c["a"], idx, values, c["axis"], modes=(c["mode"],), unique=c["unique"], di=di, dv=dv, misalign=c["misalign"])


def cand_count(rng, lib, limit, force):
    shape = draw_shape(rng, limit // 2, force, zero=0.06)
    if rng.random() < 0.5:
        op, dt = "searchsorted", ALL[int(rng.integers(0, 4))]
        budget = lib.count_plan("searchsorted", dt, [1000], [1], 4)[2][4]
        bins = int(pick(rng, [0, 1, 2, 63, 1000, budget, budget + 1, 5 * budget + 7]))
    else:
        op, dt = "bincount", INTS[int(rng.integers(0, 2))]
        K = lib.count_plan("bincount", np.int64, [1000], [1], 4)[2][3]
        bins = int(pick(rng, [1, 2, 7, 256, 1000, K, K + 1, 5 * K + 3]))
    v = draw_view(rng, shape, dt, pick_z(rng, shape, force), force, plain=bool(rng.random() < 0.25))
    word = lib.count_plan(op, dt, list(shape), list(v.strides), bins)[0]
    row = op + " " + flagged(["NONE", "LDS", "GLOBAL"][word & 0xff], word, [(sma.COUNT_COPY, "COPY")])
    return dict(fam="count", row=row, views=[v], op=op, bins=bins, mode=str(pick(rng, t_cnt.MODES)), index=str(pick(rng, t_cnt.KINDS)),
                trouble=bool(rng.random() < 0.1), misalign=int(rng.integers(0, 2)), what=f"{op} with {bins} {'edges' if op == 'searchsorted' else 'bins'}")


def vals_count(c, rng):
    v = c["views"][0]
    seed, n = int(rng.integers(1 << 20)), prod(v.wshape)
    if c["op"] == "searchsorted":
        c["edges"] = t_cnt.make_edges(v.dtype.type, c["bins"], seed)
        return [t_cnt.probes(v.dtype.type, c["edges"], n, seed + 1)]
    if c["trouble"] and n:
        return [t_cnt.trouble_ids(n, c["bins"], v.dtype.type, seed)]
    return [t_cnt.make_ids(c["index"], n, c["bins"], v.dtype.type, seed)]


def run_count(lib, c, ops):
    x, dx = ops[0]
    if c["op"] == "searchsorted":
        t_cnt.check_searchsorted(lib, c["edges"], x, dx=dx, misalign=c["misalign"], public=True)
    else:
        t_cnt.check_bincount(lib, x, c["bins"], modes=(c["mode"],), di=dx, misalign=c["misalign"])


def cand_select(rng, lib, limit, force):
    dt = ALL[int(rng.integers(0, 4))]
    shape = draw_shape(rng, limit // 4, force, zero=0.06)
    cmp = str(pick(rng, t_sel.CMP_NAMES))
    v = draw_view(rng, shape, dt, pick_z(rng, shape, force), force, plain=bool(rng.random() < 0.3))
    views, rhs = [v], None
    if cmp != "nonzero":
        rhs = "scalar"
        if rng.random() < 0.4:
            rhs = "array"
            views.append(draw_view(rng, shape, dt, pick_z(rng, shape, None, 0.1), None, plain=bool(rng.random() < 0.5)))
    src = None
    if rng.random() < 0.6:
        src = len(views)
        views.append(draw_view(rng, shape, t_sel.other_width(dt), pick_z(rng, shape, None, 0.1), None, plain=bool(rng.random() < 0.5)))
    word = lib.select_plan("values" if src else "index", dt, list(shape), list(v.strides), list(views[1].strides) if rhs == "array" else None,
                           list(views[src].strides) if src else None, cmp=sma.CMPS[cmp])[0]
    row = flagged(["NONE", "ONE", "TILES", "DENSE"][word & 0xff], word, [(sma.SELECT_COPY, "COPY")])
    return dict(fam="select", row=row, views=views, cmp=cmp, rhs=rhs, src=src, scalar=int(rng.integers(-2, 3)), misalign=int(rng.integers(0, 2)),
                data=str(pick(rng, ["specials", "ties", "ties"])), what=f"select {cmp} {rhs or ''}{' with values' if src else ''}")


def vals_select(c, rng):
    out = []
    for k, v in enumerate(c["views"]):
        seed, dt = int(rng.integers(1 << 20)), v.dtype.type
        if k == c["src"]:
            out.append(t_sort.continuous(v.wshape, dt, seed))
        elif c["data"] == "specials":
            out.append(t_sel.specials(dt, prod(v.wshape), seed, c["scalar"]).reshape(v.wshape))
        else:
            out.append(t_sort.ties(v.wshape, dt, seed))
    return out


def run_select(lib, c, ops):
    x, dx = ops[0]
    rhs_host, drhs = (ops[1] if c["rhs"] == "array" else (c["scalar"] if c["rhs"] else None, None))
    src, dsrc = ops[c["src"]] if c["src"] else (None, None)
    t_sel.check_compaction(lib, c["cmp"], x, rhs_host, dx=dx, drhs=drhs, src=src, dsrc=dsrc, misalign=c["misalign"])


def cand_runs(rng, lib, limit, force):
    dt = ALL[int(rng.integers(0, 4))]
    shape = draw_shape(rng, min(limit, 1 << 18), force, zero=0.06)
    v = draw_view(rng, shape, dt, pick_z(rng, shape, force), force)
    outputs = int(pick(rng, [t_unq.ALL, t_unq.ALL, t_unq.V, t_unq.V | t_unq.C, t_unq.V | t_unq.INV, t_unq.V | t_unq.I]))
    row = ["NONE", "ONE", "TILES"][lib.runs_plan(dt, prod(shape), outputs)[0]]
    tile = lib.runs_plan(dt, 1000)[2][1]
    return dict(fam="runs", row=row, views=[v], outputs=outputs, equal_nan=bool(rng.random() < 0.6), tile=tile, pattern=str(pick(rng, t_unq.PATTERNS)),
                nans=bool(np.dtype(dt).kind == "f" and rng.random() < 0.25), what=f"unique outputs {outputs}")


def vals_runs(c, rng):
    v = c["views"][0]
    n, dt = prod(v.wshape), v.dtype.type
    x = t_unq.keys_of(c["pattern"], n, c["tile"], 16 // v.dtype.itemsize, dt, int(rng.integers(1 << 20)))
    if c["nans"] and n:
        x[rng.integers(0, n, size=max(1, n // 50))] = rng.choice(t_unq.nans(dt), size=max(1, n // 50))
    return [x]


def run_runs(lib, c, ops):
    x, dx = ops[0]
    flat = np.ascontiguousarray(x).reshape(-1)
    en = c["equal_nan"]
    if flat.size:
        t_unq.check_both(lib, flat, en, c["outputs"])
    # the public form, on the view itself
    got = lib.unique(dx, return_index=True, return_inverse=True, return_counts=True, equal_nan=en)
    want = t_unq.np_unique(flat, en)
    total = want[t_unq.V].size
    assert got[2].shape == x.shape and all(g.shape == (total,) for g in (got[0], got[1], got[3]))
    t_unq.compare({t_unq.V: got[0].numpy(), t_unq.I: got[1].numpy(), t_unq.INV: got[2].numpy().reshape(-1), t_unq.C: got[3].numpy()}, want, flat, total,
                  (c["what"], "unique of the view"))


def cand_convert(rng, lib, limit, force):
    src, dst = ALL[int(rng.integers(0, 4))], ALL[int(rng.integers(0, 4))]
    shape = draw_shape(rng, limit, force)
    v = draw_view(rng, shape, src, pick_z(rng, shape, force), force, plain=bool(force in (None, TRAITS[0], TRAITS[4], TRAITS[5]) and rng.random() < 0.3))
    row = ["NONE", "DENSE", "ROWS", "STAGED", "COPY"][lib.convert_plan(src, dst, list(shape), list(v.strides))[0]]
    return dict(fam="convert", row=row, views=[v], dst=dst, edges=bool(rng.random() < 0.3), out=bool(rng.random() < 0.3), what=f"astype {name_of(dst)}")


def vals_convert(c, rng):
    v = c["views"][0]
    n = prod(v.wshape)
    if c["edges"] and n:
        e = (t_cvt.float_edges if v.dtype.kind == "f" else t_cvt.int_edges)(v.dtype)
        return [np.resize(np.roll(e, int(rng.integers(0, e.size))), n)]
    return [t_cvt.random_values(v.dtype, n, rng)]


def run_convert(lib, c, ops):
    x, dx = ops[0]
    out = lib.empty(x.shape, c["dst"]) if c["out"] else None
    got = lib.astype(dx, c["dst"], out=out)
    assert out is None or got is out
    t_cvt.check(got.numpy(), np.array(x), c["dst"], c["what"])


CAND = dict(reduce=cand_reduce, scan=cand_scan, arg=cand_arg, sort=cand_sort, topk=cand_topk, softmax=cand_softmax, take=cand_take, scatter=cand_scatter,
            count=cand_count, select=cand_select, runs=cand_runs, convert=cand_convert)
VALS = dict(reduce=vals_reduce, scan=vals_scan, arg=vals_arg, sort=vals_sorted_kind, topk=vals_sorted_kind, softmax=vals_softmax, take=vals_take,
            scatter=vals_scatter, count=vals_count, select=vals_select, runs=vals_runs, convert=vals_convert)
RUN = dict(reduce=run_reduce, scan=run_scan, arg=run_arg, sort=run_sort, topk=run_topk, softmax=run_softmax, take=run_take, scatter=run_scatter,
           count=run_count, select=run_select, runs=run_runs, convert=run_convert)


def steer(rng, lib, fam, row, trait, pool, tries=600):
    """A case of `fam` whose planner answers `row`, its first view with `trait`.  Candidates are drawn until one is so; the others wait
    in `pool` (a few per row) for the turn of their own row.  The trait gives way where no candidate has it (a dense route has no
    stepped view); -> (case, was the row reached)."""
    def take(need_trait):
        for k, c in enumerate(pool.get((fam, row), ())):
            if not need_trait or trait in c["views"][0].traits:
                return pool[fam, row].pop(k)
        return None
    c = take(True)
    last = None
    for k in range(tries):
        if c is not None:
            return c, True
        limit = USUAL_ELEMS if k % 4 else MAX_ELEMS
        new = CAND[fam](rng, lib, limit, trait)
        if new is None:
            continue
        last = new
        if new["row"] == row and trait in new["views"][0].traits:
            return new, True
        waiting = pool.setdefault((fam, new["row"]), [])
        if len(waiting) < 6:
            waiting.append(new)
        if k >= tries // 2:
            c = take(False)
    return last, False


# ====================================================================================================== pipelines
# A program is a list of stages over one f32 / f64 array x (or an int32 one, xi) of (O, R) -- O * R * itemsize >= 1 MiB -- and two rows
# b, b2 of R <= 4096 elements.  Each stage: (name, family, kind of operator, issue(lib, env) -> the stage's DeviceArrays, check(env,
# got) against numpy on the DOWNLOADED outputs of the stages before it: rounding does not compound, and indices cannot differ).
# The whole program is issued and synchronised once; then issued again with every intermediate dropped (back to the pool) as soon as
# its last reader has been issued, and the final result must have the same bits: every family here promises them on every run.  Kinds: "barrier" (the axis families: they flush the recorded tiny operators and are
# ordered behind everything), "tracked" (unary, astype, where, elementwise over 4096 results: the two-queue dispatcher orders them
# by their spans), "tiny" (an elementwise operator of at most 4096 results: recorded, launched later in a batch).
def _ew(op, a, b):
    return {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}[op](a, b)


def _sorted_like(x, got_v, got_i, axis, desc):
    want_v, want_i = t_sort.reference(x, axis, desc)
    if got_i is not None:
        assert got_i.dtype == np.int64 and np.array_equal(got_i, want_i), "argsort"
    if got_v is not None:
        assert got_v.tobytes() == np.ascontiguousarray(want_v).tobytes(), "sort"


def program_softmax_topk(p):
    """tiny add -> astype (tracked) -> tracked add of the tiny row -> softmax -> topk -> take_along_axis(x, indices)"""
    k = p["k"]
    return [
        ("row", "elementwise", "tiny", lambda lib, e: lib.binary(sma.OP_ADD, e["b"], e["b2"]), lambda e, g: util.assert_same_bits(g, _ew("add", e["b"], e["b2"]), "row")),
        ("cast", "convert", "tracked", lambda lib, e: lib.astype(e["xi"], p["dt"]), lambda e, g: t_cvt.check(g, e["xi"], p["dt"], "cast")),
        ("shift", "elementwise", "tracked", lambda lib, e: lib.binary(sma.OP_ADD, e["cast"], e["row"]), lambda e, g: util.assert_same_bits(g, _ew("add", e["cast"], e["row"]), "shift")),
        ("soft", "softmax", "barrier", lambda lib, e: lib.softmax(e["shift"], 1), lambda e, g: t_sm.Reference(e["shift"], 1).check("softmax", g, "pipeline")),
        ("top", "topk", "barrier", lambda lib, e: lib.topk(e["soft"], k, 1, True), lambda e, g: t_topk.same(g, t_topk.first_k(e["soft"], k, 1, True), "pipeline topk")),
        ("picked", "take", "barrier", lambda lib, e: lib.take_along_axis(e["shift"], e["top"][1], 1, mode="clip"),
         lambda e, g: _same_bytes(g, t_take.reference(e["shift"], e["top"][1], 1, "clip")[0], "take_along_axis")),
    ]


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == np.ascontiguousarray(want).tobytes(), what


def program_argsort_take(p):
    """tiny mul -> where with that row (tracked) -> argsort -> take_along_axis, which must be the sort"""
    desc = p["desc"]
    return [
        ("row", "elementwise", "tiny", lambda lib, e: lib.binary(sma.OP_MUL, e["b"], e["b2"]), lambda e, g: util.assert_same_bits(g, _ew("mul", e["b"], e["b2"]), "row")),
        ("w", "where", "tracked", lambda lib, e: lib.where((e["x"], "gt", 0.0), e["x"], e["row"]),
         lambda e, g: _same_bytes(g, np.where(e["x"] > 0, e["x"], np.broadcast_to(e["row"], e["x"].shape)), "where")),
        ("order", "sort", "barrier", lambda lib, e: lib.argsort(e["w"], 1, desc), lambda e, g: _sorted_like(e["w"], None, g, 1, desc)),
        ("sorted", "take", "barrier", lambda lib, e: lib.take_along_axis(e["w"], e["order"], 1, mode="wrap"),
         lambda e, g: (_same_bytes(g, t_take.reference(e["w"], e["order"], 1, "wrap")[0], "take_along_axis"), _sorted_like(e["w"], g, None, 1, desc))),
    ]


def program_cumsum_max(p):
    """astype (tracked) -> cumsum -> reduce max (a result of <= 4096) -> tiny sub -> tracked sub of that row's column"""
    return [
        ("cast", "convert", "tracked", lambda lib, e: lib.astype(e["xi"], p["dt"]), lambda e, g: t_cvt.check(g, e["xi"], p["dt"], "cast")),
        ("run", "scan", "barrier", lambda lib, e: lib.scan("cumsum", e["cast"], 1), lambda e, g: t_scan.check_rounded("cumsum", e["cast"], 1, g)),
        ("top", "reduce", "barrier", lambda lib, e: lib.reduce("max", e["run"], 0, keepdims=True), lambda e, g: t_red.check("max", e["run"], (0,), g, keepdims=True)),
        ("gap", "elementwise", "tiny", lambda lib, e: lib.binary(sma.OP_SUB, e["top"], e["b"]), lambda e, g: util.assert_same_bits(g, _ew("sub", e["top"], e["b"]), "gap")),
        ("below", "elementwise", "tracked", lambda lib, e: lib.binary(sma.OP_SUB, e["run"], e["gap"]), lambda e, g: util.assert_same_bits(g, _ew("sub", e["run"], e["gap"]), "below")),
    ]


def program_exp_sum_divide(p):
    """tiny sub -> tracked sub of the row -> unary exp (tracked) -> reduce sum over the columns -> elementwise divide -> argmax"""
    return [
        ("row", "elementwise", "tiny", lambda lib, e: lib.binary(sma.OP_SUB, e["b"], e["b2"]), lambda e, g: util.assert_same_bits(g, _ew("sub", e["b"], e["b2"]), "row")),
        ("d", "elementwise", "tracked", lambda lib, e: lib.binary(sma.OP_SUB, e["x"], e["row"]), lambda e, g: util.assert_same_bits(g, _ew("sub", e["x"], e["row"]), "d")),
        ("e", "unary", "tracked", lambda lib, e: lib.unary("exp", e["d"]), lambda e, g: t_un.check_ulp("exp", e["d"], g, "pipeline exp")),
        ("s", "reduce", "barrier", lambda lib, e: lib.reduce("sum", e["e"], 1, keepdims=True), lambda e, g: t_red.check("sum", e["e"], (1,), g, keepdims=True)),
        ("q", "elementwise", "tracked", lambda lib, e: lib.binary(sma.OP_DIV, e["e"], e["s"]), lambda e, g: util.assert_same_bits(g, _ew("div", e["e"], e["s"]), "q")),
        ("best", "arg", "barrier", lambda lib, e: lib.argreduce("argmax", e["q"], 1, values=True), lambda e, g: t_arg.check("argmax", e["q"], 1, g[1], g[0])),
    ]


def program_sort_search_count(p):
    """tiny add -> sort of the row (a barrier behind a tiny) -> searchsorted of x in it -> bincount of the positions -> scatter_add into them"""
    R = p["R"]
    return [
        ("row", "elementwise", "tiny", lambda lib, e: lib.binary(sma.OP_ADD, e["b"], e["b2"]), lambda e, g: util.assert_same_bits(g, _ew("add", e["b"], e["b2"]), "row")),
        ("edges", "sort", "barrier", lambda lib, e: lib.sort(e["row"], axis=None), lambda e, g: _sorted_like(e["row"].reshape(-1), g, None, 0, False)),
        ("neg", "unary", "tracked", lambda lib, e: lib.unary("neg", e["x"]), lambda e, g: util.assert_same_bits(g, t_un.expect_exact("neg", e["x"]), "neg")),
        ("pos", "count", "barrier", lambda lib, e: lib.searchsorted(e["edges"], e["neg"], "right"),
         lambda e, g: _same_bytes(g, np.searchsorted(e["edges"], e["neg"].reshape(-1), "right").astype(np.int64).reshape(e["neg"].shape), "searchsorted")),
        ("hist", "count", "barrier", lambda lib, e: lib.bincount(e["pos"], R + 1, mode="clip"), lambda e, g: _same_bytes(g, t_cnt.expected_counts(e["pos"], R + 1, "clip")[0], "bincount")),
    ]


PROGRAMS = (program_softmax_topk, program_argsort_take, program_cumsum_max, program_exp_sum_divide, program_sort_search_count)
EDGES = ("barrier -> tracked", "tracked -> barrier", "tiny -> barrier", "barrier -> tiny", "tiny -> tracked", "barrier -> barrier", "tracked -> tracked")
PIPE_ROWS = [f"edge {e}" for e in EDGES] + [f"program {f.__name__[8:]}" for f in PROGRAMS] + ["dropped mode"]
# who reads whom (by stage name), for the edge rows and for what may be dropped once its last reader is issued
READS = {
    "softmax_topk": {"cast": (), "row": (), "shift": ("cast", "row"), "soft": ("shift",), "top": ("soft",), "picked": ("shift", "top")},
    "argsort_take": {"row": (), "w": ("row",), "order": ("w",), "sorted": ("w", "order")},
    "cumsum_max": {"cast": (), "run": ("cast",), "top": ("run",), "gap": ("top",), "below": ("run", "gap")},
    "exp_sum_divide": {"row": (), "d": ("row",), "e": ("d",), "s": ("e",), "q": ("e", "s"), "best": ("q",)},
    "sort_search_count": {"row": (), "edges": ("row",), "neg": (), "pos": ("edges", "neg"), "hist": ("pos",)},
}


def draw_pipeline(rng):
    which = int(rng.integers(0, len(PROGRAMS)))
    dt = FLOATS[int(rng.integers(0, 2))]
    R = int(pick(rng, [257, 1000, 2049, 4096]))
    O = -(-(1 << 20) // (R * np.dtype(dt).itemsize)) + int(rng.integers(0, 5))   # x holds at least 1 MiB
    p = dict(fam="pipeline", which=which, name=PROGRAMS[which].__name__[8:], dt=dt, O=O, R=R, k=int(pick(rng, [1, 5, 64, 65])), desc=bool(rng.random() < 0.5),
             seed=int(rng.integers(1 << 30)))
    p["what"] = f"pipeline {p['name']} {name_of(dt)} ({O}, {R})"
    stages = PROGRAMS[which](p)
    kinds = {s[0]: s[2] for s in stages}
    p["rows"] = {f"program {p['name']}", "dropped mode"} | {f"edge {kinds[r]} -> {kinds[n]}" for n, rs in READS[p["name"]].items() for r in rs}
    return p


def pipeline_inputs(p):
    rng = np.random.default_rng(p["seed"])
    O, R, dt = p["O"], p["R"], p["dt"]
    return dict(x=t_sm.draws((O, R), dt, 3, p["seed"]), xi=rng.integers(-9, 10, size=(O, R)).astype(np.int32), b=t_sm.draws((1, R), dt, 1, p["seed"] + 1),
                b2=t_sm.draws((1, R), dt, 1, p["seed"] + 2))


def run_pipeline(lib, p):
    stages = PROGRAMS[p["which"]](p)
    reads = READS[p["name"]]
    host = pipeline_inputs(p)
    last_reader = {}
    for n, rs in reads.items():
        for r in rs:
            last_reader[r] = n

    def issue(drop):
        env = {k: lib.to_device(v) for k, v in host.items()}
        kept = {}
        for name, _, _, fn, _ in stages:
            env[name] = fn(lib, env)
            kept[name] = env[name]
            if drop:   # an intermediate goes back to the pool as soon as its last reader has been issued
                for r, n in last_reader.items():
                    if n == name:
                        env.pop(r, None)
                        kept.pop(r, None)
        return kept

    def down(v):
        return tuple(a.numpy() for a in v) if isinstance(v, tuple) else v.numpy()

    lib.synchronize()
    kept = issue(False)    # no host wait between the stages; every intermediate alive
    lib.synchronize()
    env = dict(host)
    env.update({k: down(v) for k, v in kept.items()})
    for name, _, _, _, check in stages:   # stage k against numpy on the device's own stage k - 1
        check(env, env[name])
    final = stages[-1][0]
    again = issue(True)
    lib.synchronize()
    second = down(again[final])
    for a, b in zip(second if isinstance(second, tuple) else (second,), env[final] if isinstance(env[final], tuple) else (env[final],)):
        assert a.tobytes() == b.tobytes(), f"{final}: other bits when the intermediates are dropped as soon as they have been read"


# ====================================================================================================== the soak
def turns():
    """One round of single cases: every family as often as it has rows (at least MIN_TURNS), spread evenly."""
    slots = []
    for f in FAMILIES:
        n = max(len(ROWS[f]), MIN_TURNS)
        slots += [((k + 0.5) / n, f) for k in range(n)]
    return [f for _, f in sorted(slots)]


def cases_of(cases, seed, lib):
    """The soak's cases, in order; none touches a device."""
    rng = np.random.default_rng(seed)
    order = turns()
    taken = {f: 0 for f in FAMILIES}
    singles, pool = 0, {}
    for t in range(cases):
        if t % 5 == 4:
            yield draw_pipeline(rng)
            continue
        fam = order[singles % len(order)]
        singles += 1
        k = taken[fam]
        taken[fam] += 1
        rows = ROWS[fam]
        c, reached = steer(rng, lib, fam, rows[k % len(rows)], TRAITS[(k + k // len(rows)) % len(TRAITS)], pool)
        if c["row"] not in rows:
            raise RuntimeError(f"{fam}: the planner answers {c['row']!r}, which ROWS does not list ({c['what']} {c['views']})")
        c["steered"] = reached
        c["value_seed"] = int(rng.integers(1 << 30))
        yield c


def realise(c):
    """-> [(buffer, host view)] of a single case; the values come from the family's generator."""
    rng = np.random.default_rng(c["value_seed"])
    with np.errstate(all="ignore"):
        vals = VALS[c["fam"]](c, rng)
    return [v.host(x, rng) for v, x in zip(c["views"], vals)]


def nonfinite(c, hosts):
    """Does the numpy reference of this float case hold a NaN or an infinity?  None: not a float case."""
    floats = [x for _, x in hosts if x.dtype.kind == "f"]
    if c["fam"] == "scatter" and np.dtype(c["dt"]).kind == "f":
        floats.append(c["a"])
    if not floats or (c["fam"] == "convert" and np.dtype(c["dst"]).kind != "f") or c["fam"] == "count":
        return None
    if not all(np.isfinite(x).all() for x in floats):
        return True
    if c["fam"] == "scan" and c["kind"] == "cumprod":
        with np.errstate(all="ignore"):
            return not np.isfinite(np.cumprod(hosts[0][1].astype(np.float64), axis=c["axis"]).astype(hosts[0][1].dtype)).all()
    if c["fam"] == "convert":
        with np.errstate(all="ignore"):
            return not np.isfinite(hosts[0][1].astype(c["dst"])).all()
    return False


def describe(c):
    if c["fam"] == "pipeline":
        return c["what"]
    return f"{c['fam']} [{c['row']}] {c['what']}: " + "; ".join(repr(v) for v in c["views"])


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    plan_only = "--plan-only" in sys.argv[1:]
    cases = int(argv[0]) if len(argv) > 0 else SMOKE_CASES
    seed = int(argv[1]) if len(argv) > 1 else SMOKE_SEED
    lib = sma.load()
    if not plan_only:
        lib.set_device(0)
    stats = run(lib, cases, seed, plan_only, open(argv[2], "w") if len(argv) > 2 else None, "--keep-going" in sys.argv[1:])
    if stats is None:
        return 1
    print_tables(stats, cases, seed, plan_only)
    return 0


def run(lib, cases, seed, plan_only, trace=None, keep_going=False):
    """-> the coverage counts, or None after the first mismatch (printed; with keep_going: after the last case, if any was one)."""
    failed = 0
    stats = dict(rows={(f, r): 0 for f in FAMILIES for r in ROWS[f]}, traits={(t, f): 0 for t in TRAITS for f in FAMILIES}, pipes={r: 0 for r in PIPE_ROWS},
                 float_cases=0, nonfinite=0, largest=0, unsteered=0, done=0)
    for t, c in enumerate(cases_of(cases, seed, lib)):
        if trace:   # which case was in flight when something went wrong on the GPU
            trace.write(f"case {t}: {describe(c)}\n")
            trace.flush()
            os.fsync(trace.fileno())
        if c["fam"] == "pipeline":
            for r in c["rows"]:
                stats["pipes"][r] += 1
            stats["largest"] = max(stats["largest"], c["O"] * c["R"])
            if not plan_only and not guarded(t, seed, c, lambda: run_pipeline(lib, c)):
                if not keep_going or FATAL:
                    return None
                failed += 1
            stats["done"] += 1
            continue
        hosts = realise(c)
        stats["rows"][c["fam"], c["row"]] += 1
        for trait in c["views"][0].traits:
            stats["traits"][trait, c["fam"]] += 1
        stats["unsteered"] += not c["steered"]
        stats["largest"] = max([stats["largest"]] + [v.size for v in c["views"]] + [prod(c.get("shape", ()))])
        nf = nonfinite(c, hosts)
        if nf is not None:
            stats["float_cases"] += 1
            stats["nonfinite"] += bool(nf)
        if not plan_only:
            def one():
                bufs = [lib.to_device(buf) for buf, _ in hosts]
                RUN[c["fam"]](lib, c, [(x, d.view_like(x, buf)) for d, (buf, x) in zip(bufs, hosts)])
            if not guarded(t, seed, c, one):
                if not keep_going or FATAL:
                    return None
                failed += 1
        stats["done"] += 1
    if failed:
        print(f"{failed} cases failed")
    return None if failed else stats


FATAL = []   # an error of the HIP runtime: nothing more is started on the device


def guarded(t, seed, c, fn):
    sink = io.StringIO()   # (some comparators print their margins)
    try:
        with contextlib.redirect_stdout(sink), np.errstate(all="ignore"):
            fn()
    except AssertionError as e:
        print(f"MISMATCH case {t} seed {seed}: {describe(c)}\n{e!r}"[:4000])
        return False
    except Exception as e:  # noqa: BLE001
        if isinstance(e, sma.SmhipError) and e.code == sma.ERR_HIP:
            FATAL.append(t)
        print(f"ERROR case {t} seed {seed}: {describe(c)}\n{e!r}\n{traceback.format_exc()[-1500:]}"[:6000])
        return False
    return True


def table_lines(stats):
    lines = ["coverage (cases per planner row):"]
    lines += [f"  {n:5d}  {f} {r}" for (f, r), n in stats["rows"].items()]
    lines.append("view traits (cases whose first view has each, by family):")
    lines += [f"  {n:5d}  {t} x {f}" for (t, f), n in stats["traits"].items()]
    lines.append("pipelines (programs that contain each):")
    lines += [f"  {n:5d}  {r}" for r, n in stats["pipes"].items()]
    return lines


def print_tables(stats, cases, seed, plan_only):
    print(f"{'planned' if plan_only else 'ok'}: {stats['done']} cases, seed {seed}")
    print("\n".join(table_lines(stats)))
    print(f"float cases: {stats['float_cases']}, {stats['nonfinite']} with a NaN or an infinity in the reference; largest operand {stats['largest']} elements; "
          f"{stats['unsteered']} cases took another row than the one wanted")
    print(f"skipped {cases - stats['done']}")


if __name__ == "__main__":
    sys.exit(main())
