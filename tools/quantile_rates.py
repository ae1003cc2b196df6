"""quantile along an axis (smhip_quantile_axis) against three yardsticks in the same process, all alternating:
  1. the parent's way: the library's own sort (smhip_sort_axis, values) plus, per probability, the strided slice copies of s[j] and
     s[j + 1] and the chain lo + (hi - lo) * g that interpolates, on the same operand; timed twice per round (A and A'), so the table
     shows its own A/A spread.  rule, wherever the planner picks ROW or STREAM: quantile time <= that time * (1 + that spread), else the
     row belongs to SORT;
  2. torch.quantile(t, q, dim) (torch.median for q = 0.5 alone) on the same data, also timed twice per round; the ratio is reported, no
     bar.  torch.quantile refuses inputs above 16 M elements: such rows show "-";
  3. the library's own a * s on the same operand: fraction = (the call's algorithmic bytes / its time) / (a * s bytes / its time),
     algorithmic bytes = the operand in, Q * sizeof(T) per line out; reported, no bar.
Kernel time per call from device events, `--steps` calls after warm-up, `--rounds` rounds per row (median, min .. max).  The
probabilities: 0.5, the quartiles together, and 16 at once.

Writes profiles/quantile_rates.txt (or --out).

    python tools/quantile_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"] [--no-torch] [--rows 0,3]
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
    ("(8, 2^21)", (8, 1 << 21), 1),
    ("(1, 2^24)", (1, 1 << 24), 1),
    ("(4096, 4096) axis 0", (4096, 4096), 0),
]
PROBABILITIES = [("0.5", [0.5]), ("quartiles", [0.25, 0.5, 0.75]), ("16", [(k + 0.5) / 16 for k in range(16)])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table (bench.py's headline, branch and parent)")
    ap.add_argument("--rows", default="", help="comma-separated numbers of (shape, type) rows (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="yardsticks 1 and 3 alone")
    args = ap.parse_args()
    torch, torch_note = None, "no torch (--no-torch)"
    if not args.no_torch:  # before the library touches the device
        import torch
        if not torch.cuda.is_available():
            torch, torch_note = None, "torch %s sees no GPU in this process: yardsticks 1 and 3 alone" % torch.__version__
    table = [(label, shape, dt, axis) for dt in (np.float32, np.float64) for label, shape, axis in SHAPES]
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
    say("%-20s %-4s %-9s %-36s %24s %7s %8s %26s %6s %7s %7s %24s %6s %7s" % ("shape", "type", "q", "route (O, R, I) reads launches", "quantile us", "GB/s", "of a*s",
                                                                              "sort + slices + lerp us", "A/A", "ratio", "rule", "torch us", "A/A", "ratio"))
    rows = [int(r) for r in args.rows.split(",")] if args.rows else range(len(table))
    for ri in rows:
        label, shape, dt, axis = table[ri]
        n, esz, R = int(np.prod(shape)), np.dtype(dt).itemsize, shape[axis]
        host = np.random.default_rng(7 + ri).standard_normal(shape).astype(dt)
        a = lib.to_device(host)
        svals, scaled = lib.empty(shape, dt), lib.empty(shape, dt)
        t = torch.from_numpy(host).cuda() if torch else None
        del host
        kept = tuple(1 if d == axis else s for d, s in enumerate(shape))

        def yard():
            lib.array_scalar(sma.OP_MUL, a, 1.5, out=scaled)

        for qname, qs in PROBABILITIES:
            Q = len(qs)
            out = lib.empty((Q,) + kept, dt)
            route, launches, ori, info = lib.quantile_plan(dt, list(shape), list(a.strides), axis, qs)
            rname = {sma.QUANTILE_ROUTE_SORT: "sort", sma.QUANTILE_ROUTE_ROW: "row", sma.QUANTILE_ROUTE_COPYONLY: "copy"}[route & 0xFF] + \
                ("+stream" if route & sma.QUANTILE_STREAM else "") + ("+copy" if route & sma.QUANTILE_COPY else "")
            # the parent's way: the ranks worked out by the user, a slice of the sorted array per rank, the chain per probability
            ranks = [((R - 1) * q // 1, (R - 1) * q % 1) for q in qs]
            slices = [(sma.DeviceArray(lib, svals.base_ptr, dt, kept, svals.strides, int(j) * svals.strides[axis], svals._owner),
                       sma.DeviceArray(lib, svals.base_ptr, dt, kept, svals.strides, min(int(j) + 1, R - 1) * svals.strides[axis], svals._owner), g) for j, g in ranks]
            plo, phi, pres = [lib.empty(kept, dt) for _ in qs], [lib.empty(kept, dt) for _ in qs], [lib.empty(kept, dt) for _ in qs]

            def ours():
                lib.quantile(a, qs, axis, out=out)

            def parent():
                lib.sort(a, axis, False, out=svals)
                for k, (lo, hi, g) in enumerate(slices):
                    lib.assign(plo[k], lo)
                    if g:
                        lib.assign(phi[k], hi)
                        lib.chain(phi[k], (sma.OP_SUB, plo[k]), (sma.OP_MUL, g), (sma.OP_ADD, plo[k]), out=pres[k])

            theirs = None
            if torch and n <= 16_000_000:
                tq = torch.tensor(qs, dtype=t.dtype, device=t.device)
                theirs = (lambda: torch.median(t, dim=axis)) if qs == [0.5] else (lambda: torch.quantile(t, tq, dim=axis))

            for _ in range(args.warmup):
                ours()
                parent()
                yard()
                if theirs:
                    theirs()
            got = out.numpy().reshape(Q, -1)
            # the yardstick interpolates in T: agreement on the scale of the two neighbours, 4 eps
            close = all(np.all(np.abs(got[k] - (pres[k] if g else plo[k]).numpy().reshape(-1)) <=
                               4 * np.finfo(dt).eps * np.maximum(np.abs(plo[k].numpy().reshape(-1)), np.abs(phi[k].numpy().reshape(-1)) if g else 0))
                        for k, (_, _, g) in enumerate(slices))
            ts, ty, pa, pb, ta, tb = [], [], [], [], [], []
            for _ in range(args.rounds):
                ts.append(timeit(ours))
                pa.append(timeit(parent))
                if theirs:
                    ta.append(time_torch(theirs))
                ty.append(timeit(yard))
                pb.append(timeit(parent))
                if theirs:
                    tb.append(time_torch(theirs))
            ms, my, mp = statistics.median(ts), statistics.median(ty), statistics.median(pa + pb)
            byts = n * esz + (n // R) * Q * esz
            frac = (byts / ms) / (2 * n * esz / my)
            sp = spread_of(pa, pb)
            rule = "-" if route & 0xFF != sma.QUANTILE_ROUTE_ROW else ("ok" if ms <= mp * (1.0 + sp) else "BEHIND")
            tail = "%24s %5.1f%% %7.2f" % (med(ta + tb), spread_of(ta, tb) * 100.0, statistics.median(ta + tb) / ms) if theirs else "%24s %6s %7s" % ("-", "-", "-")
            say("%-20s %-4s %-9s %-36s %24s %7.0f %7.1f%% %26s %5.1f%% %7.2f %7s %s%s" %
                (label, np.dtype(dt).name[0] + str(esz * 8), qname, "%s %s %d %d" % (rname, ori, info[2], launches), med(ts), byts / ms * 1e-3, frac * 100.0, med(pa + pb),
                 sp * 100.0, mp / ms, rule, tail, "" if close else "  VALUES DIFFER FROM SORT + SLICES + LERP"))
            del out, slices, plo, phi, pres
        del a, svals, scaled, t
        lib.pool_trim()
        if torch:
            torch.cuda.empty_cache()
    say("ratio = the yardstick's time / quantile's time; A/A = the spread between the yardstick's two interleaved series; rule (ROW and STREAM rows): quantile time <=")
    say("(sort + slices + lerp) time * (1 + its A/A), else the shape belongs to SORT.  of a*s = the call's algorithmic bytes (operand in, Q * sizeof(T) per line out) per")
    say("second over those of a * s.  reads = how often the route reads the operand at most.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
