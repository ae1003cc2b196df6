"""where / flatnonzero / select (smhip_where, smhip_select) against the library's own `a * s` at the same size and against torch on
the same values in the same process (torch.where, torch.nonzero, torch.masked_select), the three alternating.  Kernel time per call from
device events, `--steps` calls of the C ABI (arguments marshalled once) after warm-up, `--rounds` rounds per row (median, min .. max).

where, three forms:  relu      where(x > 0, x, 0)        1 read + 1 write
                     four      where(x > y, a, b)        4 reads + 1 write
                     in place  where(x > 0, x, 0) -> x   1 read + 1 write
flatnonzero / select with 1 %, 50 % and 100 % of the elements selected (x uniform in [-1, 1), the threshold chosen for the share;
select's source is x itself).  The compaction is given its capacity (the count numpy finds), so no call waits for the stream; torch's
nonzero and masked_select do wait, and write the mask: that is their design's cost, as reading x twice is this one's.

"of peak" = the call's algorithmic bytes per second over 8.0 TB/s (the HBM peak of the data sheet).  where: every read stream and the
result.  flatnonzero: x TWICE and 8 bytes per selected element.  select: x twice, and the selected elements read and written.

    python tools/select_rates.py [--steps K] [--rounds N] [--out FILE] [--sizes 20,24,28] [--no-torch]

Writes profiles/select_rates.txt (or --out).
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
SHARES = (("1 %", 0.98), ("50 %", 0.0), ("100 %", -2.0))


def med(ts):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(ts), min(ts), max(ts)) if ts else "-"


class Bench:
    def __init__(self, args):
        self.args = args
        self.torch, self.torch_note = None, "no torch"
        if not args.no_torch:  # before the library touches the device
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

    def series(self, ours, theirs, scale):
        """ours / theirs / `a * s`, alternating -> three lists of us"""
        for _ in range(self.args.warmup):
            ours()
            scale()
            if theirs:
                theirs()
        to, tt, ts = [], [], []
        for _ in range(self.args.rounds):
            to.append(self.timeit(ours))
            ts.append(self.timeit(scale))
            if theirs:
                tt.append(self.time_torch(theirs))
        return to, tt, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="20,24,28", help="log2 of the element counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    b = Bench(args)
    lib, torch = b.lib, b.torch
    say("%s%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us" %
        (lib.version(), "; torch " + torch.__version__ if torch else "; " + b.torch_note, args.steps, args.warmup, args.rounds))
    say("%-30s %-4s %6s %-10s %26s %7s %8s %26s %8s %26s %7s" % ("row", "type", "log2 n", "route, l.", "smhip us", "GB/s", "of peak", "a * s us", "of peak", "torch us", "ratio"))
    routes = {sma.SELECT_ROUTE_ONE: "one", sma.SELECT_ROUTE_TILES: "tiles", sma.SELECT_ROUTE_DENSE: "dense"}
    for dt in (np.float32, np.float64):
        esz, sdt = np.dtype(dt).itemsize, sma.DTYPES[np.dtype(dt)]
        for log2n in [int(v) for v in args.sizes.split(",")]:
            n = 1 << log2n
            x = (np.random.default_rng(log2n).random(n, dtype=dt) * 2 - 1).astype(dt)
            dx = lib.to_device(x)
            dy, da, db, dout = (lib.empty((n,), dt) for _ in range(4))
            for dst, f in ((dy, -0.5), (da, 2.0), (db, 3.0)):
                lib.array_scalar(sma.OP_MUL, dx, f, out=dst)
            sv = np.array([1.5], dt)
            scale_args = (C.c_int(sma.OP_MUL), C.c_int(sdt), C.c_void_p(dx.ptr), sv.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.c_void_p(dout.ptr))
            scale = lambda: lib.c.smhip_array_scalar(*scale_args)  # noqa: E731
            assert scale() == 0, lib.c.smhip_last_error().decode()
            zero = np.zeros(1, dt)
            zp, sh, one = zero.ctypes.data_as(C.c_void_p), sma._i64([n]), sma._i64([1])
            if torch:
                tx = torch.from_numpy(x).cuda()
                ty, ta, tb = tx * -0.5, tx * 2.0, tx * 3.0
                tz = torch.zeros((), dtype=tx.dtype, device="cuda")

            def report(label, plan, nbytes, ours, theirs):
                to, tt, ts = b.series(ours, theirs, scale)
                mo, msc = statistics.median(to), statistics.median(ts)
                rate, srate = nbytes / (mo * 1e-6), 2 * n * esz / (msc * 1e-6)
                say("%-30s %-4s %6d %-10s %26s %7.0f %7.1f%% %26s %7.1f%% %26s %7s" %
                    (label, np.dtype(dt).name[0] + str(esz * 8), log2n, "%s, %d" % (routes[plan[0] & 0xff], plan[1]), med(to), rate * 1e-9, rate / HBM_PEAK * 100.0,
                     med(ts), srate / HBM_PEAK * 100.0, med(tt), "%.2f" % (statistics.median(tt) / mo) if tt else "-"))

            # ---- where
            def where_args(y, a, b_, out):
                return (C.c_int(sma.CMP_GT), C.c_int(sdt), C.c_void_p(dx.ptr), one, C.c_void_p(y.ptr if y else 0), one if y else None, zp,
                        C.c_void_p(a.ptr), one, None, C.c_void_p(b_.ptr if b_ else 0), one if b_ else None, None if b_ else zp, sh, C.c_int(1), C.c_void_p(out.ptr))
            forms = (("where(x > 0, x, 0)", where_args(None, dx, None, dout), 2, (lambda: torch.where(tx > 0, tx, tz)) if torch else None),
                     ("where(x > y, a, b)", where_args(dy, da, db, dout), 5, (lambda: torch.where(tx > ty, ta, tb)) if torch else None),
                     ("where(x > 0, x, 0) in place", where_args(None, dx, None, dx), 2, (lambda: torch.where(tx > 0, tx, tz, out=tx)) if torch else None))
            for label, wargs, streams, theirs in forms:
                four = [1] if streams == 5 else None
                plan = lib.select_plan("where", dt, [n], [1], four, [1], four)
                ours = lambda wargs=wargs: lib.c.smhip_where(*wargs)  # noqa: E731
                assert ours() == 0, lib.c.smhip_last_error().decode()
                report(label, plan, streams * n * esz, ours, theirs)
            lib.upload(dx.ptr, x)   # the in-place form has clipped it
            if torch:
                tx = torch.from_numpy(x).cuda()
            # ---- flatnonzero / select
            for share, t in SHARES:
                k = int(np.count_nonzero(x > dt(t)))
                tv = np.array([t], dt)
                idx, vals = lib.empty((max(k, 1),), np.int64), lib.empty((max(k, 1),), dt)
                common = (C.c_int(sma.CMP_GT), C.c_int(sdt), C.c_void_p(dx.ptr), one, C.c_void_p(0), None, tv.ctypes.data_as(C.c_void_p), sh, C.c_int(1))
                fargs = (C.c_int(sma.SELECT_INDEX),) + common + (C.c_void_p(0), None, C.c_int(0), C.c_void_p(idx.ptr), C.c_int64(k), C.c_void_p(0))
                sargs = (C.c_int(sma.SELECT_VALUES),) + common + (C.c_void_p(dx.ptr), one, C.c_int(esz), C.c_void_p(vals.ptr), C.c_int64(k), C.c_void_p(0))
                plan = lib.select_plan("index", dt, [n], [1])
                for label, cargs, nbytes, theirs in (("flatnonzero, %s selected" % share, fargs, 2 * n * esz + 8 * k, (lambda: torch.nonzero(tx > t)) if torch else None),
                                                     ("select, %s selected" % share, sargs, 2 * n * esz + 2 * k * esz, (lambda: torch.masked_select(tx, tx > t)) if torch else None)):
                    ours = lambda cargs=cargs: lib.c.smhip_select(*cargs)  # noqa: E731
                    assert ours() == 0, lib.c.smhip_last_error().decode()
                    report(label, plan, nbytes, ours, theirs)
                del idx, vals
            del dx, dy, da, db, dout
            if torch:
                del tx, ty, ta, tb
                torch.cuda.empty_cache()
            lib.pool_trim()
    say("ratio = torch time / smhip time.  torch: torch.where(x > 0, x, 0), torch.where(x > y, a, b), torch.where(..., out=x); torch.nonzero(x > t);")
    say("torch.masked_select(x, x > t) -- the last two write the mask, count, and wait for the stream inside the call.")
    say("a * s = smhip_array_scalar(MUL) over the same x into a result of its own, between the two; its of peak counts 1 read + 1 write.")
    say("of peak = algorithmic bytes per second over 8.0 TB/s: where -- the read streams and the result; flatnonzero -- x twice + 8 bytes per selected")
    say("element; select -- x twice + the selected elements read and written.")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
