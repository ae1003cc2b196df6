"""sort / argsort along an axis (smhip_sort_axis) against two yardsticks in the same process, the three alternating:
  1. torch.sort(t, dim, stable=True) on the same data (it always produces values and indices); timed twice per round (A and A'),
     so the table shows the yardstick's own A/A spread beside the ratio.  goal (lines of at most K elements): sort time <=
     torch time * (1 + that spread);
  2. the library's own a * s on the same operand: fraction = (the sort's algorithmic bytes / its time) / (a * s bytes / its time),
     algorithmic bytes = the operand in, the values and / or int64 positions out.
Kernel time per call from device events, `--steps` calls after warm-up, `--rounds` rounds per row (median, min .. max).  The COPY
shape also gets its staging copy and its two scatters timed on their own (smhip_copy_strided with the same strides).

Writes profiles/sort_rates.txt (or --out).

    python tools/sort_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"] [--no-torch]
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

SHAPES = [  # label, shape, axis
    ("(512, 1000)", (512, 1000), 1),
    ("(4096, 4096)", (4096, 4096), 1),
    ("(2^20, 64)", (1 << 20, 64), 1),
    ("(2^16, 37)", (1 << 16, 37), 1),
    ("(8, 2^21)", (8, 1 << 21), 1),
    ("(1, 2^24)", (1, 1 << 24), 1),
    ("(4096, 4096) axis 0", (4096, 4096), 0),
]
TABLE = [(label, shape, dt, axis) for dt in (np.float32, np.float64) for label, shape, axis in SHAPES]
CALLS = ("sort", "argsort", "both")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table (bench.py's headline, branch and parent)")
    ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="yardstick 2 alone")
    args = ap.parse_args()
    torch, torch_note = None, "no torch (--no-torch)"
    if not args.no_torch:  # before the library touches the device
        import torch
        if not torch.cuda.is_available():
            torch, torch_note = None, "torch %s sees no GPU in this process: yardstick 2 alone" % torch.__version__
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

    def time_torch(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps * 1000.0

    def med(ts):
        return "%.1f (%.1f .. %.1f)" % (statistics.median(ts), min(ts), max(ts))

    say("%s%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us" %
        (lib.version(), "; torch " + torch.__version__ if torch else "; " + torch_note, args.steps, args.warmup, args.rounds))
    say("%-20s %-4s %-8s %-32s %24s %7s %8s %24s %7s %7s %8s" % ("shape", "type", "call", "route (O, R, I) K launches", "smhip us", "GB/s", "of a*s",
                                                                 "torch.sort us", "A/A", "ratio", "goal"))
    rows = [int(r) for r in args.rows.split(",")] if args.rows else range(len(TABLE))
    for ri in rows:
        label, shape, dt, axis = TABLE[ri]
        n, esz = int(np.prod(shape)), np.dtype(dt).itemsize
        host = np.random.default_rng(7 + ri).standard_normal(shape).astype(dt)
        a = lib.to_device(host)
        vals, idx, scaled = lib.empty(shape, dt), lib.empty(shape, np.int64), lib.empty(shape, dt)
        t = torch.from_numpy(host).cuda() if torch else None
        del host
        route, launches, ori, chunk = lib.sort_plan(dt, list(shape), list(a.strides), axis)
        rname = "row" + ("+merge" if route & sma.SORT_MERGE else "") + ("+copy" if route & sma.SORT_COPY else "")

        def yard():
            lib.array_scalar(sma.OP_MUL, a, 1.5, out=scaled)

        todo = [(c, None) for c in CALLS]
        if route & sma.SORT_COPY:  # the staging copy and the scatters on their own: the same strided copies the call makes
            perm = [d for d in range(len(shape)) if d != axis] + [axis]
            st = [0] * len(shape)
            acc = 1
            for d in reversed(perm):
                st[d], acc = acc, acc * shape[d]
            todo += [("stage-in", (a, vals, list(a.strides), st)), ("scatter", (vals, scaled, st, list(a.strides))), ("scatter i64", (idx, idx, st, list(a.strides)))]
        for call, copy in todo:
            if copy:
                src, dst, ss, ds = copy
                if src is dst:
                    dst = lib.empty(shape, np.int64)
                code = sma.DTYPES[src.dtype]

                def ours():
                    lib._ck(lib.c.smhip_copy_strided(C.c_int(code), C.c_void_p(src.ptr), sma._i64(ss), C.c_void_p(dst.ptr), sma._i64(ds), sma._i64(shape),
                                                     C.c_int(len(shape))))
                byts = 2 * n * src.dtype.itemsize
            else:
                def ours():
                    if call == "sort":
                        lib.sort(a, axis, out=vals)
                    elif call == "argsort":
                        lib.argsort(a, axis, out=idx)
                    else:
                        lib._sort(a, axis, False, True, True, vals, idx)
                byts = n * esz + (n * esz if call != "argsort" else 0) + (8 * n if call != "sort" else 0)

            def theirs():
                torch.sort(t, dim=axis, stable=True)

            use_torch = torch is not None and not copy
            for _ in range(args.warmup):
                ours()
                yard()
                if use_torch:
                    theirs()
            ts, ty, ta, tb = [], [], [], []
            for _ in range(args.rounds):
                ts.append(timeit(ours))
                if use_torch:
                    ta.append(time_torch(theirs))
                ty.append(timeit(yard))
                if use_torch:
                    tb.append(time_torch(theirs))
            ms, my = statistics.median(ts), statistics.median(ty)
            frac = (byts / ms) / (2 * n * esz / my)
            if use_torch:
                mt = statistics.median(ta + tb)
                spread = abs(statistics.median(ta) / statistics.median(tb) - 1.0)
                ratio = mt / ms
                goal = "-" if route & sma.SORT_MERGE else ("ok" if ms <= mt * (1.0 + spread) else "SLOWER")
                tail = "%24s %6.1f%% %7.2f %8s" % (med(ta + tb), spread * 100.0, ratio, goal)
            else:
                tail = "%24s %7s %7s %8s" % ("-", "-", "-", "-")
            say("%-20s %-4s %-8s %-32s %24s %7.0f %7.1f%% %s" % (label, np.dtype(dt).name[0] + str(esz * 8), call, "%s %s %d %d" % (rname, ori, chunk, launches),
                                                             med(ts), byts / ms * 1e-3, frac * 100.0, tail))
        del a, vals, idx, scaled, t
        lib.pool_trim()
        if torch:
            torch.cuda.empty_cache()
    say("ratio = torch.sort time / smhip time (torch.sort always returns values and indices); A/A = the spread between torch's two interleaved series;")
    say("goal (lines of at most K elements): smhip time <= torch time * (1 + A/A).  of a*s = the call's algorithmic bytes per second over those of a * s.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
