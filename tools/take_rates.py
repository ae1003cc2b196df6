"""take / take_along_axis (smhip_take_axis) against torch on the same tensors in the same process, the two alternating:
torch.take_along_dim for the LINE and DIRECT rows, torch.index_select for the ROWS rows.  torch's call is timed twice per round
(A and A'), so the table shows the yardstick's own A/A spread beside the ratio; goal: smhip time <= torch time * (1 + that
spread).  The DIRECT rows set no bar.  Kernel time per call from device events, `--steps` calls after warm-up, `--rounds` rounds
per row (median, min .. max).  Index mode: clip (asynchronous; torch checks its indices on the device as well).

"of peak" = the call's algorithmic bytes per second over 8.0 TB/s (the HBM peak of the data sheet): the index bytes read once,
the output bytes written once, and a's bytes the lesser of its size and what the J indices pick.

    python tools/take_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"] [--rows 0,1,..] [--no-torch]
    python tools/take_rates.py --crossover [--lines N]
                                                LINE against DIRECT on (N, 1000) f32 (N = 512 by default) with J in {1, 5, 50,
                                                1000}: the sweep behind the planner's `LINE when J >= R / c`.  Each route is
                                                forced in a child process of its own with SMHIP_TAKE_LINE_RATIO (0 = never LINE,
                                                2^30 = whenever the line fits); the children run one after the other.

Writes profiles/take_rates.txt (or --out); --crossover appends its table to the same file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import simplemath_amd as sma  # noqa: E402

HBM_PEAK = 8.0e12
ROUTES = {sma.TAKE_ROUTE_NONE: "none", sma.TAKE_ROUTE_LINE: "line", sma.TAKE_ROUTE_ROWS: "rows", sma.TAKE_ROUTE_DIRECT: "direct"}


def table():
    """label, kind ('along': a full index array, 'take': 1-D ids), a's shape, axis, J, how the indices are drawn, dtype"""
    rows = []
    for dt in (np.float32, np.float64):
        rows.append(("(512, 1000) J=1000 perm", "along", (512, 1000), 1, 1000, "perm", dt))
        for J in (1, 5, 50):
            rows.append(("(512, 1000) J=%d" % J, "along", (512, 1000), 1, J, "random", dt))
        rows.append(("(4096, 4096) axis 1 perm", "along", (4096, 4096), 1, 4096, "perm", dt))
        rows.append(("(4096, 4096) axis 0 perm", "along", (4096, 4096), 0, 4096, "perm", dt))
    rows.append(("table (2^20, 256), 2^18 ids", "take", (1 << 20, 256), 0, 1 << 18, "random", np.float32))
    rows.append(("table (50000, 64), 2^20 ids", "take", (50000, 64), 0, 1 << 20, "random", np.float32))
    rows.append(("1-D 2^26, 2^24 positions", "take", (1 << 26,), 0, 1 << 24, "random", np.float32))
    return rows


def draw(kind, shape, axis, J, how, seed):
    rng = np.random.default_rng(seed)
    R = shape[axis]
    if kind == "take":
        return rng.integers(0, R, size=J).astype(np.int64)
    ishape = list(shape)
    ishape[axis] = J
    if how == "perm":  # a permutation of the axis per line
        return np.argsort(rng.random(ishape, dtype=np.float32), axis=axis).astype(np.int64)
    return rng.integers(0, R, size=ishape).astype(np.int64)


def algorithmic_bytes(kind, shape, axis, J, esz):
    n_out = int(np.prod(shape)) // shape[axis] * J
    n_idx = J if kind == "take" else n_out
    return n_idx * 8 + n_out * esz + min(int(np.prod(shape)), n_out) * esz


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

    def row(self, kind, shape, axis, J, how, dt, seed):
        """-> (route text, our times, torch times A, torch times A')"""
        lib, torch = self.lib, self.torch
        host = np.random.default_rng(seed).standard_normal(shape).astype(dt)
        ids = draw(kind, shape, axis, J, how, seed + 1)
        a, di = lib.to_device(host), lib.to_device(ids)
        oshape = list(shape)
        oshape[axis] = J
        out = lib.empty(oshape, dt)
        if kind == "take":
            si = [0] * len(shape)
            si[axis] = 1
        else:
            si = list(di.strides)
        route, launches, oji, K = lib.take_plan(dt, list(a.strides), shape[axis], si, oshape, axis)
        text = "%s%s %s %d" % (ROUTES[route & 0xff], "+copy" if route & sma.TAKE_COPY else "", oji, launches)
        ours = (lambda: lib.take(a, di, axis, mode="clip", out=out)) if kind == "take" else (lambda: lib.take_along_axis(a, di, axis, mode="clip", out=out))
        theirs = None
        if torch:
            t, ti = torch.from_numpy(host).cuda(), torch.from_numpy(ids).cuda()
            tout = torch.empty(oshape, dtype=t.dtype, device="cuda")
            theirs = (lambda: torch.index_select(t, axis, ti, out=tout)) if kind == "take" else (lambda: torch.take_along_dim(t, ti, axis, out=tout))
        del host, ids
        for _ in range(self.args.warmup):
            ours()
            if theirs:
                theirs()
        ts, ta, tb = [], [], []
        for _ in range(self.args.rounds):
            ts.append(self.timeit(ours))
            if theirs:
                ta.append(self.time_torch(theirs))
            ts.append(self.timeit(ours))
            if theirs:
                tb.append(self.time_torch(theirs))
        del a, di, out
        lib.pool_trim()
        if torch:
            del t, ti, tout
            torch.cuda.empty_cache()
        return text, ts, ta, tb


def med(ts):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(ts), min(ts), max(ts))


def crossover_child(args):
    """One route forced by the environment: times of (lines, 1000) f32 with each J, as one JSON line."""
    b = Bench(args, False)
    res = {}
    for J in (1, 5, 50, 1000):
        text, ts, _, _ = b.row("along", (args.lines, 1000), 1, J, "perm" if J == 1000 else "random", np.float32, 100 + J)
        res[str(J)] = (text, ts)
    print("CROSSOVER " + json.dumps(res), flush=True)


def crossover(args, say):
    got = {}
    for name, c in (("DIRECT", "0"), ("LINE", str(1 << 30))):
        env = dict(os.environ, SMHIP_TAKE_LINE_RATIO=c)
        cmd = [sys.executable, os.path.abspath(__file__), "--crossover-child", "--lines", str(args.lines), "--steps", str(args.steps), "--rounds", str(args.rounds),
               "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CROSSOVER ")]
        if r.returncode != 0 or not line:
            raise SystemExit("crossover child %s failed: %s" % (name, (r.stdout + r.stderr)[-2000:]))
        got[name] = json.loads(line[0][len("CROSSOVER "):])
    say("LINE against DIRECT on (%d, 1000) f32, R = 1000, each route forced with SMHIP_TAKE_LINE_RATIO in a process of its own; "
        "us per call, median (min .. max)" % args.lines)
    say("%-6s %-8s %28s %28s %10s" % ("J", "R / J", "LINE us", "DIRECT us", "DIRECT/LINE"))
    for J in ("1", "5", "50", "1000"):
        tl, td = got["LINE"][J][1], got["DIRECT"][J][1]
        assert got["LINE"][J][0].startswith("line") and got["DIRECT"][J][0].startswith("direct"), (got["LINE"][J][0], got["DIRECT"][J][0])
        say("%-6s %-8.0f %28s %28s %10.2f" % (J, 1000 / int(J), med(tl), med(td), statistics.median(td) / statistics.median(tl)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "take_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table (bench.py's headline, branch and parent)")
    ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--lines", type=int, default=512, help="--crossover: the number of lines of 1000 elements (default 512)")
    ap.add_argument("--crossover-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.crossover_child:
        return crossover_child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.crossover:
        crossover(args, say)
        mode = "a"
    else:
        mode = "w"
        b = Bench(args, not args.no_torch)
        say("%s%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us; mode clip" %
            (b.lib.version(), "; torch " + b.torch.__version__ if b.torch else "; " + b.torch_note, args.steps, args.warmup, args.rounds))
        say("%-30s %-4s %-34s %26s %8s %8s %26s %7s %7s %8s" % ("row", "type", "route (O, J, I) launches", "smhip us", "GB/s", "of peak", "torch us", "A/A", "ratio", "goal"))
        rows = table()
        for ri in ([int(r) for r in args.rows.split(",")] if args.rows else range(len(rows))):
            label, kind, shape, axis, J, how, dt = rows[ri]
            esz = np.dtype(dt).itemsize
            text, ts, ta, tb = b.row(kind, shape, axis, J, how, dt, 7 + ri)
            ms = statistics.median(ts)
            rate = algorithmic_bytes(kind, shape, axis, J, esz) / (ms * 1e-6)
            if ta:
                mt = statistics.median(ta + tb)
                spread = abs(statistics.median(ta) / statistics.median(tb) - 1.0)
                goal = "-" if text.startswith("direct") else ("ok" if ms <= mt * (1.0 + spread) else "SLOWER")
                tail = "%26s %6.1f%% %7.2f %8s" % (med(ta + tb), spread * 100.0, mt / ms, goal)
            else:
                tail = "%26s %7s %7s %8s" % ("-", "-", "-", "-")
            say("%-30s %-4s %-34s %26s %8.0f %7.1f%% %s" % (label, np.dtype(dt).name[0] + str(esz * 8), text, med(ts), rate * 1e-9, rate / HBM_PEAK * 100.0, tail))
        say("ratio = torch time / smhip time; A/A = the spread between torch's two interleaved series; goal: smhip time <= torch time * (1 + A/A); the DIRECT rows set no bar.")
        say("of peak = algorithmic bytes (indices in, result out, a's bytes the lesser of its size and what is picked) per second over 8.0 TB/s.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, mode) as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
