"""searchsorted / bincount / histogram (smhip_searchsorted, smhip_bincount, smhip_histogram) against torch on the same tensors in the
same process, the two alternating: torch.bincount, torch.histc (equal bins; the explicit-edges rows are held against it too, torch.histogram having no
device form) and torch.searchsorted.  torch's call is timed twice per round (A and A'), so the table shows the yardstick's own A/A
spread beside the ratio; goal on the LDS-route rows: smhip time <= torch time * (1 + that spread).  For bincount torch's time under
torch.use_deterministic_algorithms(True) stands next to it, and a second column times this tree's own index_add spelling of the same
bincount, `index_add(zeros, ids, 1, 0)`: the 256-bin rows must beat that column.  Kernel time per call from device events, `--steps`
calls of the C ABI (arguments marshalled once) after warm-up, `--rounds` rounds per row (median, min .. max).  Index mode: clip.

"of peak" = the call's algorithmic bytes per second over 8.0 TB/s (the HBM peak of the data sheet): the input for bincount and
histogram, the input plus the int64 result for searchsorted.

    python tools/count_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"] [--rows 0,1,..] [--no-torch]

Writes profiles/count_rates.txt (or --out).
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
ROUTES = {sma.COUNT_ROUTE_NONE: "none", sma.COUNT_ROUTE_LDS: "lds", sma.COUNT_ROUTE_GLOBAL: "global"}


def table(K):
    """label, what, dtype, n, bins (edges for searchsorted), how the values are drawn, the uniform table"""
    rows = [("bincount 256 bins, 2^24 uniform", "bincount", np.int64, 1 << 24, 256, "uniform", False),
            ("bincount 256 bins, 2^24 one bin", "bincount", np.int64, 1 << 24, 256, "same", False),
            ("bincount K bins, 2^24 uniform", "bincount", np.int64, 1 << 24, K, "uniform", False),
            ("bincount K + 1 bins, 2^24 uniform", "bincount", np.int64, 1 << 24, K + 1, "uniform", False),
            ("bincount 2^20 bins, 2^24 uniform", "bincount", np.int64, 1 << 24, 1 << 20, "uniform", False),
            ("bincount 2^20 bins, 2^24 one bin", "bincount", np.int64, 1 << 24, 1 << 20, "same", False)]
    for dt in (np.float32, np.float64):
        for bins in (256, 4096):
            rows.append(("histogram %d bins, 2^26, range" % bins, "histogram", dt, 1 << 26, bins, "uniform", True))
            rows.append(("histogram %d bins, 2^26, edges" % bins, "histogram", dt, 1 << 26, bins, "uniform", False))
    for dt in (np.float32, np.float64):
        for edges in (256, 1 << 20):
            rows.append(("searchsorted 2^26 in %d edges" % edges, "searchsorted", dt, 1 << 26, edges, "uniform", False))
    return rows


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

    def row(self, what, dt, n, bins, how, uniform, seed):
        """-> (route text, our times, torch times A, torch times A', torch's deterministic times, the index_add spelling's times)"""
        lib, torch = self.lib, self.torch
        rng = np.random.default_rng(seed)
        one, zero = C.c_int64(1), C.c_int64(0)
        theirs = spelled = None
        keep = []
        if what == "bincount":
            ids = np.full(n, bins // 3, np.int64) if how == "same" else rng.integers(0, bins, size=n).astype(np.int64)
            dx, out = lib.to_device(ids), lib.empty((bins,), np.int64)
            argv = (C.c_int(sma.INDEX_CLIP), C.c_int(sma.I64), C.c_void_p(dx.ptr), sma._i64([n]), sma._i64([1]), C.c_int(1), C.c_int64(bins), C.c_void_p(out.ptr),
                    C.c_void_p(0))
            call = lib.c.smhip_bincount
            # the spelling the README used to give: index_add of the constant 1 onto a zeroed target (the zeroing is part of it)
            target, ones = lib.empty((bins,), np.int64), lib.to_device(np.ones(1, np.int64))
            fill = (C.c_int(sma.I64), C.c_void_p(target.ptr), C.byref(zero), C.c_size_t(bins))
            sargv = (C.c_int(sma.SCATTER_ADD), C.c_int(sma.INDEX_CLIP), C.c_int(0), C.c_int(sma.I64), C.c_void_p(target.ptr), sma._i64([bins]), C.c_int(1), C.c_int(0),
                     C.c_void_p(dx.ptr), sma._i64([1]), C.c_void_p(ones.ptr), sma._i64([0]), C.c_int64(n), C.c_void_p(0))
            keep += [target, ones, one]

            def spelled():
                lib.c.smhip_fill(*fill)
                return lib.c.smhip_scatter_axis(*sargv)
            if torch:
                ti = torch.from_numpy(ids).cuda()
                theirs = lambda: torch.bincount(ti, minlength=bins)  # noqa: E731
            plan = lib.count_plan("bincount", np.int64, [n], [1], bins)
        else:
            x = rng.uniform(-4.0, 4.0, size=n).astype(dt)
            dx = lib.to_device(x)
            if what == "histogram":
                edges = lib.histogram_edges(bins, -4.0, 4.0, dt)
                de, out = lib.to_device(edges), lib.empty((bins,), np.int64)
                argv = (C.c_int(sma.HISTOGRAM_UNIFORM if uniform else 0), C.c_int(sma.DTYPES[np.dtype(dt)]), C.c_void_p(dx.ptr), sma._i64([n]), sma._i64([1]), C.c_int(1),
                        C.c_void_p(de.ptr), C.c_int64(bins), C.c_double(-4.0), C.c_double(4.0), C.c_void_p(out.ptr))
                call = lib.c.smhip_histogram
                if torch:
                    tx = torch.from_numpy(x).cuda()
                    theirs = lambda: torch.histc(tx, bins=bins, min=-4.0, max=4.0)  # noqa: E731
                plan = lib.count_plan("histogram", dt, [n], [1], bins, uniform=uniform)
            else:
                edges = np.sort(rng.uniform(-4.0, 4.0, size=bins).astype(dt))
                de, out = lib.to_device(edges), lib.empty((n,), np.int64)
                argv = (C.c_int(sma.SIDE_RIGHT), C.c_int(sma.DTYPES[np.dtype(dt)]), C.c_void_p(de.ptr), C.c_int64(bins), C.c_void_p(dx.ptr), sma._i64([n]), sma._i64([1]),
                        C.c_int(1), C.c_void_p(out.ptr))
                call = lib.c.smhip_searchsorted
                if torch:
                    tx, te = torch.from_numpy(x).cuda(), torch.from_numpy(edges).cuda()
                    tout = torch.empty(n, dtype=torch.int64, device="cuda")
                    theirs = lambda: torch.searchsorted(te, tx, right=True, out=tout)  # noqa: E731
                plan = lib.count_plan("searchsorted", dt, [n], [1], bins)
            keep.append(de)
        text = "%s%s wg %d x %d r%d, %d" % (ROUTES[plan[0] & 0xff], "+copy" if plan[0] & sma.COUNT_COPY else "", plan[2][0], plan[2][1], plan[2][2], plan[1])
        assert call(*argv) == 0, lib.c.smhip_last_error().decode()
        ours = lambda: call(*argv)  # noqa: E731
        for _ in range(self.args.warmup):
            ours()
            if theirs:
                theirs()
        ts, ta, tb, td, tsp = [], [], [], [], []
        for _ in range(self.args.rounds):
            ts.append(self.timeit(ours))
            if theirs:
                ta.append(self.time_torch(theirs))
            ts.append(self.timeit(ours))
            if theirs:
                tb.append(self.time_torch(theirs))
        if spelled:  # one call first: with every id in one bin the sorted route takes seconds, and is then timed by that call alone
            steps, self.args.steps = self.args.steps, 1
            tsp = [self.timeit(spelled)]
            self.args.steps = steps
            if tsp[0] < 50e3:
                tsp = [self.timeit(spelled) for _ in range(max(1, self.args.rounds // 2))]
        if theirs and what == "bincount":
            try:
                torch.use_deterministic_algorithms(True)
                theirs()
                td = [self.time_torch(theirs) for _ in range(self.args.rounds)]
            except Exception as e:  # torch has no deterministic form of this call
                td = []
                print("  (deterministic torch: %s)" % str(e).splitlines()[0][:120], flush=True)
            finally:
                torch.use_deterministic_algorithms(False)
        del dx, out, keep
        lib.pool_trim()
        if torch:
            torch.cuda.empty_cache()
        return text, ts, ta, tb, td, tsp


def med(ts):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table (bench.py's headline, branch and parent)")
    ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    b = Bench(args, not args.no_torch)
    K = b.lib.count_plan("bincount", np.int64, [1000], [1], 4)[2][3]
    say("%s%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us; mode clip; K = %d" %
        (b.lib.version(), "; torch " + b.torch.__version__ if b.torch else "; " + b.torch_note, args.steps, args.warmup, args.rounds, K))
    say("%-36s %-4s %-34s %28s %7s %8s %28s %7s %7s %7s %12s %14s" % ("row", "type", "route wg x entries replicas, launches", "smhip us", "GB/s", "of peak", "torch us",
                                                                      "A/A", "ratio", "goal", "torch det us", "index_add us"))
    rows = table(K)
    for ri in ([int(r) for r in args.rows.split(",")] if args.rows else range(len(rows))):
        label, what, dt, n, bins, how, uniform = rows[ri]
        esz = np.dtype(dt).itemsize
        text, ts, ta, tb, td, tsp = b.row(what, dt, n, bins, how, uniform, 7 + ri)
        ms = statistics.median(ts)
        rate = n * (esz + (8 if what == "searchsorted" else 0)) / (ms * 1e-6)
        if ta:
            mt = statistics.median(ta + tb)
            spread = abs(statistics.median(ta) / statistics.median(tb) - 1.0)
            best = min([mt] + ([statistics.median(td)] if td else []))  # torch's faster form
            goal = "-" if not text.startswith("lds") else ("ok" if ms <= best * (1.0 + spread) else "SLOWER")
            tail = "%28s %6.1f%% %7.2f %7s %12s" % (med(ta + tb), spread * 100.0, mt / ms, goal, "%.1f" % statistics.median(td) if td else "-")
        else:
            tail = "%28s %7s %7s %7s %12s" % ("-", "-", "-", "-", "-")
        say("%-36s %-4s %-34s %28s %7.0f %7.1f%% %s %14s" % (label, np.dtype(dt).name[0] + str(esz * 8), text, med(ts), rate * 1e-9, rate / HBM_PEAK * 100.0, tail,
                                                            "%.1f" % statistics.median(tsp) if tsp else "-"))
    say("ratio = torch time / smhip time; A/A = the spread between torch's two interleaved series; goal (LDS-route rows): smhip time <= torch's faster form * (1 + A/A).")
    say("torch: torch.bincount / torch.histc / torch.searchsorted(right=True); torch det us = torch.bincount under torch.use_deterministic_algorithms(True), median.")
    say("index_add us = this tree's smhip_fill of the target + smhip_scatter_axis(ADD) of the constant 1 over the same ids (the sorted route, unchanged by this family).")
    say("of peak = algorithmic bytes (the input; searchsorted: plus the int64 result) per second over 8.0 TB/s.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
