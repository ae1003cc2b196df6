"""softmax, log_softmax and logsumexp along an axis (smhip_softmax_axis) against three yardsticks in the same process, all alternating:
  1. the parent's way, the four-call recipe through the library: reduce max (keepdims), the chain exp(x - m), reduce sum (keepdims),
     divide (log_softmax: (x - m) - log(sum); logsumexp: m + log(sum) -- the same two reductions and the exp chain).  goal, on every
     held route (reads == 1): the fused call takes less time; by bytes it should take a third (2 against 6 * sizeof(T) per element);
  2. torch.softmax / torch.log_softmax / torch.logsumexp on the same values; the ratio is reported, no bar;
  3. the library's own a * s over the same array, which moves the same 2 * sizeof(T) bytes per element: the fused call's share of
     that rate (algorithmic bytes: the operand in, the result out); reported, no bar.
Kernel time per call from device events, the arguments of the recipe's chains marshalled once, `--steps` calls after warm-up,
`--rounds` alternating rounds per row (median, min .. max).

Writes profiles/softmax_rates.txt (or --out).

    python tools/softmax_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"] [--no-torch] [--rows 0,3]
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
    ("(65536, 128)", (65536, 128), 1),
    ("(8, 2^22)", (8, 1 << 22), 1),
    ("(4096, 4097)", (4096, 4097), 1),
    ("(4096, 4096) axis 0", (4096, 4096), 0),
    ("(64, 1000, 64) axis 1", (64, 1000, 64), 1),
]
KINDS = ("softmax", "log_softmax", "logsumexp")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_rates.txt"))
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

    say("%s%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us" %
        (lib.version(), "; torch " + torch.__version__ if torch else "; " + torch_note, args.steps, args.warmup, args.rounds))
    say("%-22s %-4s %-12s %-40s %22s %7s %8s %24s %7s %7s %24s %7s" % ("shape", "type", "kind", "route (O, R, I) reads levels launches", "fused us", "GB/s", "of a*s",
                                                                        "recipe us", "ratio", "goal", "torch us", "ratio"))
    rows = [int(r) for r in args.rows.split(",")] if args.rows else range(len(table))
    for ri in rows:
        label, shape, dt, axis = table[ri]
        n, esz, R = int(np.prod(shape)), np.dtype(dt).itemsize, shape[axis]
        host = np.random.default_rng(7 + ri).standard_normal(shape).astype(dt) * dt(10)
        a = lib.to_device(host)
        t = torch.from_numpy(host).cuda() if torch else None
        del host
        keep = tuple(1 if d == axis else s for d, s in enumerate(shape))
        m, s, logs = lib.empty(keep, dt), lib.empty(keep, dt), lib.empty(keep, dt)
        e, res, scaled = lib.empty(shape, dt), lib.empty(shape, dt), lib.empty(shape, dt)
        # the recipe's chains, marshalled once
        exp_chain, _ = lib.chain_call(a, ("sub", m), ("exp",), out=e)
        divide, _ = lib.chain_call(e, ("div", s), out=res)
        log_of_sum, _ = lib.chain_call(s, ("log",), out=logs)
        shifted, _ = lib.chain_call(a, ("sub", m), ("sub", logs), out=res)
        lse_chain, _ = lib.chain_call(s, ("log",), ("add", m), out=logs)

        def reductions():
            lib.reduce("max", a, axis, keepdims=True, out=m)
            exp_chain()
            lib.reduce("sum", e, axis, keepdims=True, out=s)

        def recipe_softmax():
            reductions()
            divide()

        def recipe_log_softmax():
            reductions()
            log_of_sum()
            shifted()

        def recipe_logsumexp():
            reductions()
            lse_chain()

        def yard():
            lib.array_scalar(sma.OP_MUL, a, 1.5, out=scaled)

        recipes = dict(softmax=recipe_softmax, log_softmax=recipe_log_softmax, logsumexp=recipe_logsumexp)
        for kind in KINDS:
            out = lib.empty(shape if kind != "logsumexp" else tuple(sz for d, sz in enumerate(shape) if d != axis), dt)
            route, launches, ori, info = lib.softmax_plan(kind, dt, list(shape), list(a.strides), axis)
            rname = ("row" if route & 0xFF == sma.SOFTMAX_ROUTE_ROW else "column") + ("+split" if route & sma.SOFTMAX_SPLIT else "") + ("+copy" if route & sma.SOFTMAX_COPY else "")
            fused_fn = getattr(lib, kind)

            def ours():
                fused_fn(a, axis, out=out)

            parent = recipes[kind]
            if torch:
                theirs = {"softmax": lambda: torch.softmax(t, axis), "log_softmax": lambda: torch.log_softmax(t, axis), "logsumexp": lambda: torch.logsumexp(t, axis)}[kind]
            for _ in range(args.warmup):
                ours()
                parent()
                yard()
                if torch:
                    theirs()
            got = out.numpy().astype(np.float64).reshape(-1)
            want = (res if kind != "logsumexp" else logs).numpy().astype(np.float64).reshape(-1)
            worst = float(np.max(np.abs(got - want) / (np.abs(want) + 1e-30))) if kind == "softmax" else float(np.max(np.abs(got - want)))
            ts, ty, tp, tt = [], [], [], []
            for _ in range(args.rounds):
                ts.append(timeit(ours))
                tp.append(timeit(parent))
                if torch:
                    tt.append(time_torch(theirs))
                ty.append(timeit(yard))
            ms, my, mp = statistics.median(ts), statistics.median(ty), statistics.median(tp)
            byts = n * esz + out.size * esz
            frac = (byts / ms) / (2 * n * esz / my)
            goal = "-" if info[1] != 1 else ("ok" if ms < mp else "SLOWER") + (" >1/2" if ms > 0.5 * mp else "")
            tail = "%24s %7.2f" % (med(tt), statistics.median(tt) / ms) if torch else "%24s %7s" % ("-", "-")
            say("%-22s %-4s %-12s %-40s %22s %7.0f %7.1f%% %24s %7.2f %7s %s   max diff from the recipe %.2e" %
                (label, np.dtype(dt).name[0] + str(esz * 8), kind, "%s %s %d %d %d" % (rname, ori, info[1], info[2], launches), med(ts), byts / ms * 1e-3, frac * 100.0,
                 med(tp), mp / ms, goal, tail, worst))
            del out
        del a, m, s, logs, e, res, scaled, t, exp_chain, divide, log_of_sum, shifted, lse_chain
        lib.pool_trim()
        if torch:
            torch.cuda.empty_cache()
    say("ratio = the yardstick's time / the fused call's time; goal (held routes, reads == 1): fused time < recipe time, '>1/2' where it takes more than half of it.")
    say("of a*s = the call's algorithmic bytes (operand in, result out) per second over those of a * s on the same array.  max diff: relative for softmax, absolute for the others.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
