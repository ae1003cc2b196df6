"""smhip_runs (the kernel behind unique / unique_consecutive) against the library's own select compaction at 50 % over the same n and
against torch on the same values in the same process (torch.unique_consecutive, torch.unique), the three alternating.  Kernel time per
call from device events, `--steps` calls of the C ABI (arguments marshalled once) after warm-up, `--rounds` rounds per row (median,
min .. max).

runs    SORTED input with U = 1 %, 50 % and 100 % of n runs (s[i] = the (i // d)-th value of the type, d = 100, 2, 1), f32 and i64:
          values                     values_out alone                          algorithmic bytes: s twice + U elements
          values counts inverse      what unique_consecutive asks, no `order`  s twice + inverse (8 n) + U * (element + 8)
          all four by order          what unique asks behind its sort          s twice + order + inverse (16 n) + U * (element + 16)
        `order` is the permutation i -> i * 2654435761 mod n (n a power of two): scattered like a sort's positions, cheap to make; the
        inverse is then n scattered 8-byte stores, which torch.unique_consecutive has no counterpart of (no torch column).
        The call is given its capacity U, so it never waits for the stream; torch.unique_consecutive does.
select  smhip_select(VALUES, x > 0) over n uniform values of the same type, half of them selected: UNCHANGED code that moves the same
        algorithmic bytes as `runs, values, U = n / 2` -- x twice plus the written half.  The yardstick: "x select" = runs time / its time.
unique  the whole lib.unique(x) -- sort, count, one wait, runs -- over the same values shuffled, at the sizes in --unique-sizes, against
        torch.unique(x) (and with all three extras against torch.unique(x, return_inverse=True, return_counts=True); torch has no index),
        and beside it its first step alone: lib.sort(x, axis=None) without and with positions against torch.sort.

    python tools/unique_rates.py [--steps K] [--rounds N] [--out FILE] [--sizes 20,24,28] [--unique-sizes 20,24] [--no-torch]

Writes profiles/unique_rates.txt (or --out).
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplemath_amd as sma  # noqa: E402
from select_rates import HBM_PEAK, Bench, med  # noqa: E402

SHARES = (("1 %", 100), ("50 %", 2), ("100 %", 1))


def sorted_values(dt, n, d):
    """n ascending values of `dt` in runs of d: the (i // d)-th value above 1.0 (f32: its bit pattern counts up) or above -n / 2 (i64)."""
    ids = np.arange(n, dtype=np.int64) // d
    if np.dtype(dt) == np.float32:
        return (ids + 0x3F800000).astype(np.uint32).view(np.float32)
    return ids - n // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="20,24,28", help="log2 of the element counts of the runs rows")
    ap.add_argument("--unique-sizes", default="20,24", help="log2 of the element counts of the whole-unique rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unique_rates.txt"))
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
    say("%-34s %-4s %6s %-9s %26s %7s %8s %26s %9s %26s %7s" % ("row", "type", "log2 n", "route, l.", "smhip us", "GB/s", "of peak", "select 50 % us", "x select", "torch us", "ratio"))
    routes = {sma.RUNS_ROUTE_ONE: "one", sma.RUNS_ROUTE_TILES: "tiles"}
    unique_sizes = [int(v) for v in args.unique_sizes.split(",") if v]
    for dt in (np.float32, np.int64):
        esz, sdt = np.dtype(dt).itemsize, sma.DTYPES[np.dtype(dt)]
        name = np.dtype(dt).name[0] + str(esz * 8)
        for log2n in [int(v) for v in args.sizes.split(",")]:
            n = 1 << log2n
            rng = np.random.default_rng(log2n)
            # ---- the yardstick: select at 50 % over n values of this type
            y = (rng.random(n, dtype=np.float32) * 2 - 1) if np.dtype(dt) == np.float32 else rng.integers(-1 << 40, 1 << 40, size=n)
            y = y.astype(dt)
            k = int(np.count_nonzero(y > 0))
            dy, dsel = lib.to_device(y), lib.empty((max(k, 1),), dt)
            zero, one, sh = np.zeros(1, dt), sma._i64([1]), sma._i64([n])
            sel_args = (C.c_int(sma.SELECT_VALUES), C.c_int(sma.CMP_GT), C.c_int(sdt), C.c_void_p(dy.ptr), one, C.c_void_p(0), None, zero.ctypes.data_as(C.c_void_p), sh,
                        C.c_int(1), C.c_void_p(dy.ptr), one, C.c_int(esz), C.c_void_p(dsel.ptr), C.c_int64(k), C.c_void_p(0))
            select = lambda: lib.c.smhip_select(*sel_args)  # noqa: E731
            assert select() == 0, lib.c.smhip_last_error().decode()
            del y
            order = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(n - 1)).astype(np.int64)
            dorder, dinverse = lib.to_device(order), lib.empty((n,), np.int64)
            del order

            def report(label, plan, nbytes, ours, theirs):
                to, tt, ts = b.series(ours, theirs, select)
                mo, ms = statistics.median(to), statistics.median(ts)
                rate = nbytes / (mo * 1e-6)
                say("%-34s %-4s %6d %-9s %26s %7.0f %7.1f%% %26s %9.2f %26s %7s" %
                    (label, name, log2n, "%s, %d" % (routes.get(plan[0], "-"), plan[1]), med(to), rate * 1e-9, rate / HBM_PEAK * 100.0, med(ts), mo / ms, med(tt),
                     "%.2f" % (statistics.median(tt) / mo) if tt else "-"))

            for share, d in SHARES:
                s = sorted_values(dt, n, d)
                U = -(-n // d)
                ds = lib.to_device(s)
                dvalues, dindex, dcounts = lib.empty((U,), dt), lib.empty((U,), np.int64), lib.empty((U,), np.int64)
                head = (C.c_int(0), C.c_int(sdt), C.c_void_p(ds.ptr), C.c_int64(n))
                vargs = head + (C.c_void_p(0), C.c_void_p(dvalues.ptr), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_int64(U), C.c_void_p(0))
                aargs = head + (C.c_void_p(dorder.ptr), C.c_void_p(dvalues.ptr), C.c_void_p(dindex.ptr), C.c_void_p(dcounts.ptr), C.c_void_p(dinverse.ptr), C.c_int64(U),
                                C.c_void_p(0))
                if torch:
                    ts_ = torch.from_numpy(s).cuda()
                cargs_ = head + (C.c_void_p(0), C.c_void_p(dvalues.ptr), C.c_void_p(0), C.c_void_p(dcounts.ptr), C.c_void_p(dinverse.ptr), C.c_int64(U), C.c_void_p(0))
                rows = (("runs, values, U = %s of n" % share, vargs, sma.RUNS_VALUES, 2 * n * esz + U * esz, (lambda: torch.unique_consecutive(ts_)) if torch else None),
                        ("runs, values counts inverse, %s" % share, cargs_, 13, 2 * n * esz + 8 * n + U * (esz + 8),
                         (lambda: torch.unique_consecutive(ts_, return_inverse=True, return_counts=True)) if torch else None),
                        ("runs, all four by order, %s" % share, aargs, 15, 2 * n * esz + 16 * n + U * (esz + 16), None))
                for label, cargs, outputs, nbytes, theirs in rows:
                    ours = lambda cargs=cargs: lib.c.smhip_runs(*cargs)  # noqa: E731
                    assert ours() == 0, lib.c.smhip_last_error().decode()
                    report(label, lib.runs_plan(dt, n, outputs), nbytes, ours, theirs)
                if share == "50 %":   # what the timed calls wrote is what numpy finds
                    lib.synchronize()
                    assert dvalues.numpy().tobytes() == s[::d].tobytes() and (dcounts.numpy() == d).all()
                # ---- the whole unique over the same values, shuffled
                if log2n in unique_sizes and share != "100 %":
                    x = rng.permutation(s)
                    dx = lib.to_device(x)
                    if torch:
                        tx = torch.from_numpy(x).cuda()
                    assert lib.unique(dx).shape == (U,)
                    dsorted, dwhere = lib.empty((n,), dt), lib.empty((n,), np.int64)
                    report("sort(x), the unique's first step", (0, 0), 2 * n * esz, lambda: lib.sort(dx, axis=None, out=dsorted), (lambda: torch.sort(tx)) if torch else None)
                    report("sort(x) with positions", (0, 0), 2 * n * esz + 8 * n, lambda: lib._sort(dx, None, False, True, True, dsorted, dwhere),
                           (lambda: torch.sort(tx, stable=True)) if torch else None)
                    del dsorted, dwhere
                    report("unique(x), U = %s of n" % share, (0, 0), n * esz + U * esz, lambda: lib.unique(dx), (lambda: torch.unique(tx)) if torch else None)
                    report("unique(x) + index, inverse, counts", (0, 0), n * esz + 8 * n + U * (esz + 16),
                           lambda: lib.unique(dx, return_index=True, return_inverse=True, return_counts=True),
                           (lambda: torch.unique(tx, return_inverse=True, return_counts=True)) if torch else None)
                    del dx, x
                    if torch:
                        del tx
                del ds, dvalues, dindex, dcounts, s
                if torch:
                    del ts_
                    torch.cuda.empty_cache()
                lib.pool_trim()
            del dy, dsel, dorder, dinverse
            lib.pool_trim()
    say("x select = smhip time / the time of smhip_select(VALUES, x > 0) at 50 % over n values of the same type, alternating with it (unchanged code:")
    say("the yardstick).  `runs, values, U = 50 %` moves the same algorithmic bytes as that select: s twice plus the written half.")
    say("ratio = torch time / smhip time.  torch: unique_consecutive(s), unique_consecutive(s, return_inverse=True, return_counts=True), unique(x),")
    say("unique(x, return_inverse=True, return_counts=True) -- each waits for the stream inside the call; smhip_runs is given its capacity and does not.")
    say("lib.unique waits once.  of peak = algorithmic bytes per second over 8.0 TB/s: values -- s twice + U elements; values counts inverse -- s twice +")
    say("8 n + U * (element + 8); all four by order -- s twice + order + inverse + U * (element + 16), the inverse being n SCATTERED 8-byte stores;")
    say("sort -- x and the result (and the positions); unique -- x once + the results (the sort's own traffic is not counted: a whole-call figure).")
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
