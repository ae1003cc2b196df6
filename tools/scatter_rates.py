"""put_along_axis / put / scatter_add / index_add (smhip_scatter_axis) against torch on the same tensors in the same process, the two
alternating: torch.Tensor.scatter_ for the put_along_axis rows, scatter_add_ / index_add_ for the ADD rows, index_copy_ for the
unique put of whole rows.  torch's call is timed twice per round (A and A'), so the table shows the yardstick's own A/A spread beside
the ratio; goal on the UNIQUE routes: smhip time <= torch time * (1 + that spread).  The sorted routes set no bar: torch's adds are
atomic and not reproducible, ours are the same bits on every run; where torch offers a deterministic form
(torch.use_deterministic_algorithms(True)) its time is recorded next to the ratio.  Kernel time per call from device events,
`--steps` calls of the C ABI (arguments marshalled once) after warm-up, `--rounds` rounds per row (median, min .. max).  Index mode: clip (asynchronous).

"of peak" = the call's algorithmic bytes per second over 8.0 TB/s (the HBM peak of the data sheet): the index bytes read once, the
values read once, the destinations written once (ADD: and read once), a destination counted once however many entries name it.

    python tools/scatter_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"] [--rows 0,1,..] [--no-torch]

Writes profiles/scatter_rates.txt (or --out).
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import simplemath_amd as sma  # noqa: E402

HBM_PEAK = 8.0e12
ROUTES = {sma.SCATTER_ROUTE_NONE: "none", sma.SCATTER_ROUTE_DIRECT: "direct", sma.SCATTER_ROUTE_ROWS: "rows", sma.SCATTER_ROUTE_SORTED: "sorted",
          sma.SCATTER_ROUTE_SORTED_ROWS: "sorted_rows"}


def table():
    """label, form ('along': a full index array, 'ids': 1-D ids), kind, the target's shape, axis, J, how the indices are drawn,
    unique, scalar values, dtype"""
    rows = []
    for dt in (np.float32, np.float64):
        rows.append(("(512, 1000) perm, unique", "along", "put", (512, 1000), 1, 1000, "perm", True, False, dt))
        for axis in (1, 0):
            for unique in (True, False):
                rows.append(("(4096, 4096) axis %d perm%s" % (axis, ", unique" if unique else ""), "along", "put", (4096, 4096), axis, 4096, "perm", unique, False, dt))
        rows.append(("(4096, 4096) random, add", "along", "add", (4096, 4096), 1, 4096, "random", False, False, dt))
        rows.append(("table (50000, 64), 2^20 ids, add", "ids", "add", (50000, 64), 0, 1 << 20, "random", False, False, dt))
        rows.append(("table (2^20, 256), 2^18 ids, unique", "ids", "put", (1 << 20, 256), 0, 1 << 18, "distinct", True, False, dt))
        rows.append(("bincount 256 bins, 2^24", "ids", "add", (256,), 0, 1 << 24, "random", False, True, dt))
    return rows


def draw(form, shape, axis, J, how, seed):
    rng = np.random.default_rng(seed)
    R = shape[axis]
    if form == "ids":
        return (rng.permutation(R)[:J] if how == "distinct" else rng.integers(0, R, size=J)).astype(np.int64)
    ishape = list(shape)
    ishape[axis] = J
    if how == "perm":  # a permutation of the axis per line
        return np.argsort(rng.random(ishape, dtype=np.float32), axis=axis).astype(np.int64)
    return rng.integers(0, R, size=ishape).astype(np.int64)


def algorithmic_bytes(form, kind, shape, axis, J, scalar, esz):
    entries = int(np.prod(shape)) // shape[axis] * J
    n_idx = J if form == "ids" else entries
    touched = min(int(np.prod(shape)), entries)
    return n_idx * 8 + (1 if scalar else entries) * esz + touched * esz * (2 if kind == "add" else 1)


class Bench:
    def __init__(self, args, want_torch):
        self.args = args
        self.torch, self.torch_note = None, "no torch"
        if want_torch:  # before the library touches the device
            import torch
            if torch.cuda.is_available():
                self.torch = torch
            else:
                self.torch_note = "torch %s sees no GPU in this process" % torch.__version__
        self.lib = sma.load()
        self.lib.set_device(0)

    def timeit(self, fn):
        lib = self.lib
        e0, e1 = lib.event(), lib.event()
        lib.synchronize()
        lib.record(e0)
        for _ in range(self.args.steps):
            fn()
        lib.record(e1)
        lib.synchronize()
        t = lib.elapsed_ms(e0, e1) / self.args.steps * 1000.0
        lib.event_destroy(e0)
        lib.event_destroy(e1)
        return t

    def time_torch(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(self.args.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / self.args.steps * 1000.0

    def row(self, form, kind, shape, axis, J, how, unique, scalar, dt, seed):
        """-> (route text, our times, torch times A, torch times A', torch's deterministic times)"""
        lib, torch = self.lib, self.torch
        rng = np.random.default_rng(seed)
        ids = draw(form, shape, axis, J, how, seed + 1)
        wshape = list(shape)
        wshape[axis] = J
        vals = np.ones(1, dt) if scalar else rng.standard_normal(wshape).astype(dt)
        a, di, dv = lib.to_device(np.zeros(shape, dt)), lib.to_device(ids), lib.to_device(vals)
        if form == "ids":
            si = [0] * len(shape)
            si[axis] = 1
        else:
            si = list(di.strides)
        sv = [0] * len(shape) if scalar else list(dv.strides)
        route, launches, orji, nsorted = lib.scatter_plan(dt, shape, axis, si, sv, J, unique=unique)
        text = "%s%s %s %d" % (ROUTES[route & 0xff], "+copy" if route & sma.SCATTER_COPY else "", orji, launches)
        # the C ABI with its arguments marshalled once: the timing loop pays the call, not the binding's Python
        argv = (C.c_int(sma.SCATTER_ADD if kind == "add" else sma.SCATTER_PUT), C.c_int(sma.INDEX_CLIP), C.c_int(sma.SCATTER_UNIQUE if unique else 0),
                C.c_int(sma.DTYPES[np.dtype(dt)]), C.c_void_p(a.ptr), sma._i64(shape), C.c_int(len(shape)), C.c_int(axis), C.c_void_p(di.ptr), sma._i64(si),
                C.c_void_p(dv.ptr), sma._i64(sv), C.c_int64(J), C.c_void_p(0))
        call = lib.c.smhip_scatter_axis
        assert call(*argv) == 0, lib.c.smhip_last_error().decode()
        ours = lambda: call(*argv)  # noqa: E731
        theirs = None
        if torch:
            t, ti = torch.zeros(shape, dtype=torch.from_numpy(vals).dtype, device="cuda"), torch.from_numpy(ids).cuda()
            tv = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(vals, wshape))).cuda()  # torch wants the values in full
            if form == "along":
                theirs = (lambda: t.scatter_(axis, ti, tv)) if kind == "put" else (lambda: t.scatter_add_(axis, ti, tv))
            elif len(shape) == 1:
                theirs = lambda: t.scatter_add_(0, ti, tv)  # noqa: E731
            else:
                theirs = (lambda: t.index_copy_(axis, ti, tv)) if kind == "put" else (lambda: t.index_add_(axis, ti, tv))
        del ids, vals
        for _ in range(self.args.warmup):
            ours()
            if theirs:
                theirs()
        ts, ta, tb, td = [], [], [], []
        for _ in range(self.args.rounds):
            ts.append(self.timeit(ours))
            if theirs:
                ta.append(self.time_torch(theirs))
            ts.append(self.timeit(ours))
            if theirs:
                tb.append(self.time_torch(theirs))
        if theirs and kind == "add":
            try:
                torch.use_deterministic_algorithms(True)
                theirs()
                td = [self.time_torch(theirs) for _ in range(self.args.rounds)]
            except Exception as e:  # torch has no deterministic form of this call
                td = []
                print("  (deterministic torch: %s)" % str(e).splitlines()[0][:120], flush=True)
            finally:
                torch.use_deterministic_algorithms(False)
        del a, di, dv
        lib.pool_trim()
        if torch:
            del t, ti, tv
            torch.cuda.empty_cache()
        return text, ts, ta, tb, td


def med(ts):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scatter_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table (bench.py's headline, branch and parent)")
    ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    b = Bench(args, not args.no_torch)
    say("%s%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us; mode clip" %
        (b.lib.version(), "; torch " + b.torch.__version__ if b.torch else "; " + b.torch_note, args.steps, args.warmup, args.rounds))
    say("%-38s %-4s %-44s %30s %8s %8s %30s %7s %7s %8s %12s" % ("row", "type", "route (O, R, J, I) launches", "smhip us", "GB/s", "of peak", "torch us", "A/A", "ratio",
                                                                  "goal", "torch det us"))
    rows = table()
    for ri in ([int(r) for r in args.rows.split(",")] if args.rows else range(len(rows))):
        label, form, kind, shape, axis, J, how, unique, scalar, dt = rows[ri]
        esz = np.dtype(dt).itemsize
        text, ts, ta, tb, td = b.row(form, kind, shape, axis, J, how, unique, scalar, dt, 7 + ri)
        ms = statistics.median(ts)
        rate = algorithmic_bytes(form, kind, shape, axis, J, scalar, esz) / (ms * 1e-6)
        if ta:
            mt = statistics.median(ta + tb)
            spread = abs(statistics.median(ta) / statistics.median(tb) - 1.0)
            goal = "-" if text.startswith("sorted") else ("ok" if ms <= mt * (1.0 + spread) else "SLOWER")
            tail = "%30s %6.1f%% %7.2f %8s %12s" % (med(ta + tb), spread * 100.0, mt / ms, goal, "%.1f" % statistics.median(td) if td else "-")
        else:
            tail = "%30s %7s %7s %8s %12s" % ("-", "-", "-", "-", "-")
        say("%-38s %-4s %-44s %30s %8.0f %7.1f%% %s" % (label, np.dtype(dt).name[0] + str(esz * 8), text, med(ts), rate * 1e-9, rate / HBM_PEAK * 100.0, tail))
    say("ratio = torch time / smhip time; A/A = the spread between torch's two interleaved series; goal (unique routes only): smhip time <= torch time * (1 + A/A).")
    say("torch det us = the same torch call under torch.use_deterministic_algorithms(True), median; '-' where torch has none or the row is a PUT.")
    say("of peak = algorithmic bytes (indices in, values in, each named destination out once -- ADD: and in once) per second over 8.0 TB/s.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
