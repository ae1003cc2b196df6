"""Cumulative scans (smhip_scan_axis) against yardsticks from the library in the same process, the two alternating:
kernel time per call from HIP events, 20 calls after warm-up, five rounds per row (the median is reported, the spread shown).

    one-launch routes   against `a * s` on an array of the same bytes: it moves the same two streams
    SPLIT routes        against `sum` over the same axis of the same array PLUS `a * s` of the same bytes: launch 1 is
                        that reduction, launch 2 a two-stream pass

ratio = yardstick time / scan time; algorithmic bytes = input + output.  Writes profiles/scan_rates.txt (or --out).

    python tools/scan_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"]
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

BAR = 0.85
TABLE = [  # label, shape, dtype, axis, has a bar
    ("16384x16384 f32 axis 1", (16384, 16384), np.float32, 1, True),
    ("(2^20, 256) f32 axis 1", (1 << 20, 256), np.float32, 1, True),
    ("8192x8192 f64 axis 1", (8192, 8192), np.float64, 1, True),
    ("16384x16384 f32 axis 0", (16384, 16384), np.float32, 0, True),
    ("(4, 2^26) f32 axis 1", (4, 1 << 26), np.float32, 1, True),
    ("(2^22, 64) f32 axis 0", (1 << 22, 64), np.float32, 0, True),
    ("(2^24, 3) f32 axis 0", (1 << 24, 3), np.float32, 0, False),
    ("(2^23, 8) f32 axis 0", (1 << 23, 8), np.float32, 0, False),
    ("(2^24, 3) f32 axis 1", (1 << 24, 3), np.float32, 1, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kinds", default="cumsum,cummax")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_rates.txt"))
    ap.add_argument("--headline", default="", help="a line recorded under the table (bench.py's headline, branch and parent)")
    ap.add_argument("--rows", default="", help="comma-separated row numbers (default: all)")
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

    say("%s; %d calls per timing after %d warm-up calls, %d alternating rounds, median (min .. max) in us" %
        (lib.version(), args.steps, args.warmup, args.rounds))
    say("%-24s %-7s %-22s %7s %22s %22s %7s %6s" % ("shape", "kind", "route (O, R, I) chunk", "GB/s", "scan us", "yardstick us", "ratio", "bar"))
    rows = [int(r) for r in args.rows.split(",")] if args.rows else range(len(TABLE))
    for ri in rows:
        label, shape, dt, axis, has_bar = TABLE[ri]
        n = int(np.prod(shape))
        a = lib.empty(shape, dt)
        if dt == np.float32:
            lib._ck(lib.c.smhip_fill_uniform_f32(C.c_void_p(a.ptr), C.c_size_t(n), C.c_uint64(7), C.c_uint64(0), C.c_float(-1.0), C.c_float(1.0)))
        else:
            v = np.array([1.5], dt)
            lib._ck(lib.c.smhip_fill(C.c_int(sma.DTYPES[np.dtype(dt)]), C.c_void_p(a.ptr), v.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        out = lib.empty(shape, dt)
        scaled = lib.empty(shape, dt)
        red_shape = tuple(e for d, e in enumerate(shape) if d != axis)
        red = lib.empty(red_shape, dt)
        route, launches, ori, chunk = lib.scan_plan("cumsum", dt, list(shape), list(a.strides), axis)
        split = bool(route & sma.SCAN_SPLIT)
        rname = {sma.SCAN_ROUTE_ROW: "row", sma.SCAN_ROUTE_COLUMN: "column"}.get(route & 0xff, str(route & 0xff)) + ("+split" if split else "")
        byts = 2 * n * np.dtype(dt).itemsize
        for kind in args.kinds.split(","):
            rkind = "sum" if kind == "cumsum" else "max"

            def scan():
                lib.scan(kind, a, axis, out=out)

            def yard():
                if split:
                    lib.reduce(rkind, a, axis, out=red)
                lib.array_scalar(sma.OP_MUL, a, 1.0001, out=scaled)

            for _ in range(args.warmup):
                scan()
                yard()
            ts, ty = [], []
            for _ in range(args.rounds):
                ts.append(timeit(scan))
                ty.append(timeit(yard))
            ms, my = statistics.median(ts), statistics.median(ty)
            ratio = my / ms
            say("%-24s %-7s %-22s %7.0f %22s %22s %7.3f %6s" % (
                label, kind, "%s %s %d" % (rname, ori, chunk), byts / ms * 1e-3,
                "%.1f (%.1f .. %.1f)" % (ms, min(ts), max(ts)), "%.1f (%.1f .. %.1f)" % (my, min(ty), max(ty)), ratio,
                "-" if not has_bar else ("ok" if ratio >= BAR else "UNDER")))
        del a, out, scaled, red
        lib.pool_trim()
    say("bar: ratio >= %.2f (yardstick time / scan time); rows marked '-' are recorded without one" % BAR)
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
