"""var and standardize (smhip_moments_axes / smhip_standardize_axis) against two yardsticks in the same process, all alternating:
  1. the recipe the library offered before: sqrt(mean(pow(x - mean(x, axis, keepdims), 2), axis, keepdims)) -- a reduction, a chain
     into a full-size temporary, a reduction, a chain; four calls and two full reads of x plus the temporary's write and read;
  2. reduce SUM on the same shape, which moves the operand once.
Expectations (reported as met or missed, nothing asserted): a held ROW var (reads == 1) moves the bytes of sum and should take
within about 10 % of its time; a route with reads == 2 about twice sum; both less than the recipe.
Kernel time per call from device events, the recipe's chains marshalled once, `--steps` calls after warm-up, `--rounds` alternating
rounds per row (median, min .. max).  Algorithmic bytes: the operand in, the result out.

Writes profiles/moments_rates.txt (or --out).

    python tools/moments_rates.py [--steps K] [--rounds N] [--out FILE] [--rows 0,3]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import simplemath_amd as sma  # noqa: E402

SHAPES = [  # label, shape, dtype, axes
    ("16384x16384 axis 1", (16384, 16384), np.float32, 1),
    ("16384x16384 axis 0", (16384, 16384), np.float32, 0),
    ("(2^20, 256) axis 1", (1 << 20, 256), np.float32, 1),
    ("(1024,224,224,3) {0,1,2}", (1024, 224, 224, 3), np.float32, (0, 1, 2)),
    ("8192x8192 axis 0", (8192, 8192), np.float64, 0),
    ("8192x8192 axis 1", (8192, 8192), np.float64, 1),
]
ROUTES = {sma.MOMENTS_ROUTE_ROW: "row", sma.MOMENTS_ROUTE_COLUMN: "column", sma.MOMENTS_ROUTE_CHANNEL: "channel", sma.MOMENTS_ROUTE_UNIT: "unit"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_rates.txt"))
    ap.add_argument("--rows", default="", help="comma-separated numbers of rows (default: all)")
    args = ap.parse_args()
    lib = sma.load()
    lib.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timeit(fn):
        e0, e1 = lib.event(), lib.event()
        lib.synchronize()
        lib.record(e0)
        for _ in range(args.steps):
            fn()
        lib.record(e1)
        lib.synchronize()
        t = lib.elapsed_ms(e0, e1) / args.steps * 1000.0
        lib.event_destroy(e0)
        lib.event_destroy(e1)
        return t

    def med(ts):
        return "%.0f (%.0f .. %.0f)" % (statistics.median(ts), min(ts), max(ts))

    def name(route):
        return ROUTES[route & 0xFF] + ("+split" if route & sma.MOMENTS_SPLIT else "") + ("+copy" if route & sma.MOMENTS_COPY else "")

    say("%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us" % (lib.version(), args.steps, args.warmup, args.rounds))
    say("%-26s %-4s %-12s %-36s %20s %7s %20s %8s %20s %8s  %s" % ("shape", "type", "call", "route (O, R, I) reads launches", "us", "GB/s", "sum us", "of sum", "recipe us", "ratio", "expectation"))
    rows = [int(r) for r in args.rows.split(",")] if args.rows else range(len(SHAPES))
    for ri in rows:
        label, shape, dt, axis = SHAPES[ri]
        axes = (axis,) if isinstance(axis, int) else axis
        n, esz = int(np.prod(shape)), np.dtype(dt).itemsize
        a = lib.empty(shape, dt)
        flat = sma.DeviceArray(lib, a.base_ptr, dt, (n,), (1,), a.offset, a._owner)
        piece = (np.random.default_rng(7 + ri).standard_normal(1 << 22) * 3 + 100).astype(dt)
        dpiece = lib.to_device(piece)
        for start in range(0, n, 1 << 22):  # filled on the device piece by piece: the host never holds the whole operand
            m = min(1 << 22, n - start)
            lib.assign(sma.DeviceArray(lib, a.base_ptr, dt, (m,), (1,), a.offset + start, a._owner), sma.DeviceArray(lib, dpiece.base_ptr, dt, (m,), (1,), dpiece.offset, dpiece._owner))
        del flat, piece, dpiece
        keep = tuple(1 if d in axes else s for d, s in enumerate(shape))
        kept = tuple(s for d, s in enumerate(shape) if d not in axes)
        mean, msq, sd = lib.empty(keep, dt), lib.empty(keep, dt), lib.empty(keep, dt)
        tmp = lib.empty(shape, dt)
        squares, _ = lib.chain_call(a, ("sub", mean), ("pow", dt(2)), out=tmp)
        root, _ = lib.chain_call(msq, ("sqrt",), out=sd)
        total, var_out = lib.empty(kept, dt), lib.empty(kept, dt)

        def recipe():
            lib.reduce("mean", a, axis, keepdims=True, out=mean)
            squares()
            lib.reduce("mean", tmp, axis, keepdims=True, out=msq)
            root()

        def yard():
            lib.reduce("sum", a, axis, out=total)

        def var():
            lib.var(a, axis, out=var_out)

        calls = [("var", var, lib.moments_plan("var", dt, list(shape), list(a.strides), axis), n * esz + var_out.size * esz)]
        if isinstance(axis, int) and axis == len(shape) - 1:
            y = lib.empty(shape, dt)
            calls.append(("standardize", lambda: lib.standardize(a, axis, out=y), lib.standardize_plan(dt, list(shape), list(a.strides), axis), 2 * n * esz))
        for _ in range(args.warmup):
            recipe()
            yard()
            for _, fn, _, _ in calls:
                fn()
        got, want = lib.std(a, axis).numpy().astype(np.float64).reshape(-1), sd.numpy().astype(np.float64).reshape(-1)
        diff = float(np.max(np.abs(got - want) / np.abs(want)))
        tr, ty = [], []
        ts = [[] for _ in calls]
        for _ in range(args.rounds):
            for k, (_, fn, _, _) in enumerate(calls):
                ts[k].append(timeit(fn))
            tr.append(timeit(recipe))
            ty.append(timeit(yard))
        mr, my = statistics.median(tr), statistics.median(ty)
        for k, (what, _, (route, launches, ori, info), byts) in enumerate(calls):
            ms = statistics.median(ts[k])
            if what == "var":
                target = 1.1 if info[1] == 1 else 2.2
                verdict = "%s %.1fx sum (reads %d: <= %.1fx), %s the recipe" % ("met" if ms <= target * my and ms < mr else "MISSED", ms / my, info[1], target, "beats" if ms < mr else "SLOWER than")
            else:
                verdict = "%s the recipe (reported, no bar against sum: it writes the operand's size)" % ("beats" if ms < mr else "SLOWER than")
            say("%-26s %-4s %-12s %-36s %20s %7.0f %20s %7.2fx %20s %8.2f  %s" % (label, np.dtype(dt).name[0] + str(esz * 8), what, "%s %s %d %d" % (name(route), ori, info[1], launches), med(ts[k]),
                                                                                   byts / ms * 1e-3, med(ty), ms / my, med(tr), mr / ms, verdict))
        say("%-26s      stddev against the recipe's: max relative difference %.2e" % ("", diff))
        del a, mean, msq, sd, tmp, squares, root, total, var_out, calls
        lib.pool_trim()
    say("of sum = the call's time over reduce SUM's on the same view; ratio = the recipe's time over the call's.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
