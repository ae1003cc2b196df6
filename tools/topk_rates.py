"""topk along an axis (smhip_topk_axis, values and positions) against three yardsticks in the same process, all alternating:
  1. the parent's way: the library's own sort_with_index (smhip_sort_axis, both outputs) plus the strided copy of the first k of each,
     on the same operand; timed twice per round (A and A'), so the table shows its own A/A spread.  goal, wherever the planner picks
     ROW or TILED: topk time < that time * (1 - that spread);
  2. torch.topk(t, k, dim, largest=True, sorted=True) on the same data, also timed twice per round; the ratio is reported, no bar;
  3. the library's own a * s on the same operand: fraction = (topk's algorithmic bytes / its time) / (a * s bytes / its time),
     algorithmic bytes = the operand in, k * (sizeof(T) + 8) per line out; reported, no bar.
Kernel time per call from device events, `--steps` calls after warm-up, `--rounds` rounds per row (median, min .. max).  k runs over
1, 5, 64, kmax and kmax + 1 (clipped to the axis), kmax read from the plan.

Writes profiles/topk_rates.txt (or --out).  --sweep times the shapes that decided the planner's hand-overs instead (many lines of 128,
129, 256, 1024, 1025 and 4096 elements, k also 256 and 257): profiles/topk_handover_sweep.txt.

    python tools/topk_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"] [--no-torch] [--rows 0,3] [--sweep]
"""
import argparse
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
SWEEP = [  # --sweep: many lines either side of the planner's hand-overs (ranked | a wave per line | a workgroup per line | tiles)
    ("(2^18, 128)", (1 << 18, 128), 1),
    ("(2^18, 129)", (1 << 18, 129), 1),
    ("(2^17, 256)", (1 << 17, 256), 1),
    ("(2^16, 1024)", (1 << 16, 1024), 1),
    ("(2^16, 1025)", (1 << 16, 1025), 1),
    ("(2^14, 4096)", (1 << 14, 4096), 1),
]
SWEEP_K = (1, 5, 64, 256, 257)  # ... and of the k at which a line leaves its wave


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table (bench.py's headline, branch and parent)")
    ap.add_argument("--rows", default="", help="comma-separated numbers of (shape, type) rows (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="yardsticks 1 and 3 alone")
    ap.add_argument("--sweep", action="store_true", help="the hand-over shapes instead of the table's (profiles/topk_handover_sweep.txt)")
    args = ap.parse_args()
    torch, torch_note = None, "no torch (--no-torch)"
    if not args.no_torch:  # before the library touches the device
        import torch
        if not torch.cuda.is_available():
            torch, torch_note = None, "torch %s sees no GPU in this process: yardsticks 1 and 3 alone" % torch.__version__
    table = [(label, shape, dt, axis) for dt in (np.float32, np.float64) for label, shape, axis in (SWEEP if args.sweep else SHAPES)]
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

    def spread_of(ta, tb):
        return abs(statistics.median(ta) / statistics.median(tb) - 1.0)

    say("%s%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us" %
        (lib.version(), "; torch " + torch.__version__ if torch else "; " + torch_note, args.steps, args.warmup, args.rounds))
    say("%-20s %-4s %5s %-34s %22s %7s %8s %24s %6s %7s %7s %24s %6s %7s" % ("shape", "type", "k", "route (O, R, I) levels launches", "topk us", "GB/s", "of a*s",
                                                                             "sort + slices us", "A/A", "ratio", "goal", "torch.topk us", "A/A", "ratio"))
    rows = [int(r) for r in args.rows.split(",")] if args.rows else range(len(table))
    for ri in rows:
        label, shape, dt, axis = table[ri]
        n, esz, R = int(np.prod(shape)), np.dtype(dt).itemsize, shape[axis]
        host = np.random.default_rng(7 + ri).standard_normal(shape).astype(dt)
        a = lib.to_device(host)
        svals, sidx, scaled = lib.empty(shape, dt), lib.empty(shape, np.int64), lib.empty(shape, dt)
        t = torch.from_numpy(host).cuda() if torch else None
        del host
        kmax = lib.topk_plan(dt, list(shape), list(a.strides), axis, 1)[3][1]

        def yard():
            lib.array_scalar(sma.OP_MUL, a, 1.5, out=scaled)

        for k in sorted({min(k, R) for k in (1, 5, 64, kmax, kmax + 1) + (SWEEP_K if args.sweep else ())}):
            kshape = tuple(k if d == axis else s for d, s in enumerate(shape))
            vals, idx = lib.empty(kshape, dt), lib.empty(kshape, np.int64)
            head_v = sma.DeviceArray(lib, svals.base_ptr, dt, kshape, svals.strides, 0, svals._owner)  # the first k along the axis of the sorted arrays
            head_i = sma.DeviceArray(lib, sidx.base_ptr, np.int64, kshape, sidx.strides, 0, sidx._owner)
            pvals, pidx = lib.empty(kshape, dt), lib.empty(kshape, np.int64)
            route, launches, ori, info = lib.topk_plan(dt, list(shape), list(a.strides), axis, k)
            rname = ("sort" if route & 0xFF == sma.TOPK_ROUTE_SORT else "row") + ("+tiled" if route & sma.TOPK_TILED else "") + ("+copy" if route & sma.TOPK_COPY else "")

            def ours():
                lib.topk(a, k, axis, True, out=vals, index_out=idx)

            def parent():
                lib._sort(a, axis, True, True, True, svals, sidx)
                lib.assign(pvals, head_v)
                lib.assign(pidx, head_i)

            def theirs():
                torch.topk(t, k, dim=axis, largest=True, sorted=True)

            for _ in range(args.warmup):
                ours()
                parent()
                yard()
                if torch:
                    theirs()
            same = vals.numpy().tobytes() == pvals.numpy().tobytes() and idx.numpy().tobytes() == pidx.numpy().tobytes()
            ts, ty, pa, pb, ta, tb = [], [], [], [], [], []
            for _ in range(args.rounds):
                ts.append(timeit(ours))
                pa.append(timeit(parent))
                if torch:
                    ta.append(time_torch(theirs))
                ty.append(timeit(yard))
                pb.append(timeit(parent))
                if torch:
                    tb.append(time_torch(theirs))
            ms, my, mp = statistics.median(ts), statistics.median(ty), statistics.median(pa + pb)
            byts = n * esz + (n // R) * k * (esz + 8)
            frac = (byts / ms) / (2 * n * esz / my)
            sp = spread_of(pa, pb)
            goal = "-" if route & 0xFF == sma.TOPK_ROUTE_SORT else ("ok" if ms < mp * (1.0 - sp) else "SLOWER")
            tail = "%24s %5.1f%% %7.2f" % (med(ta + tb), spread_of(ta, tb) * 100.0, statistics.median(ta + tb) / ms) if torch else "%24s %6s %7s" % ("-", "-", "-")
            say("%-20s %-4s %5d %-34s %22s %7.0f %7.1f%% %24s %5.1f%% %7.2f %7s %s%s" %
                (label, np.dtype(dt).name[0] + str(esz * 8), k, "%s %s %d %d" % (rname, ori, info[2], launches), med(ts), byts / ms * 1e-3, frac * 100.0, med(pa + pb),
                 sp * 100.0, mp / ms, goal, tail, "" if same else "  BYTES DIFFER FROM SORT + SLICES"))
            del vals, idx, pvals, pidx, head_v, head_i
        del a, svals, sidx, scaled, t
        lib.pool_trim()
        if torch:
            torch.cuda.empty_cache()
    say("ratio = the yardstick's time / topk's time; A/A = the spread between the yardstick's two interleaved series; goal (ROW and TILED rows): topk time <")
    say("(sort + slices) time * (1 - its A/A).  of a*s = the call's algorithmic bytes (operand in, k * (sizeof(T) + 8) per line out) per second over those of a * s.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
