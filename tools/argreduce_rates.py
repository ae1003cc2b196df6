"""argmax along an axis (smhip_argreduce_axis) against the library's own max over the same axis (smhip_reduce_axes MAX) on the
SAME operand in the same process, the two alternating: kernel time per call from HIP events, 20 calls after warm-up, five
rounds per row (the median is reported, the spread shown).  argmax reads the same bytes as max and writes 8 instead of
sizeof(T) bytes per result; `+value` is the one-pass "max and where" (value_out given).

ratio = max time / argmax time; algorithmic bytes = the operand.  Writes profiles/argreduce_rates.txt (or --out).

    python tools/argreduce_rates.py [--steps K] [--rounds N] [--out FILE] [--headline "text"]
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
SHAPES = [  # label, shape, axis
    ("4096x65536 axis 1", (4096, 65536), 1),
    ("65536x4096 axis 0", (65536, 4096), 0),
    ("(4, 2^26) axis 1", (4, 1 << 26), 1),
    ("(2^24, 3) axis 0", (1 << 24, 3), 0),
    ("(2^22, 64) axis 1", (1 << 22, 64), 1),
]
TABLE = [(label, shape, dt, axis) for dt in (np.float32, np.float64) for label, shape, axis in SHAPES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "argreduce_rates.txt"))
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
    say("%-20s %-4s %-8s %-34s %7s %22s %22s %7s %6s" % ("shape", "type", "call", "route (O, R, I) chunk launches", "GB/s", "argmax us", "max us", "ratio", "bar"))
    rows = [int(r) for r in args.rows.split(",")] if args.rows else range(len(TABLE))
    for ri in rows:
        label, shape, dt, axis = TABLE[ri]
        n = int(np.prod(shape))
        a = lib.empty(shape, dt)
        if dt == np.float32:
            lib._ck(lib.c.smhip_fill_uniform_f32(C.c_void_p(a.ptr), C.c_size_t(n), C.c_uint64(7), C.c_uint64(0), C.c_float(-1.0), C.c_float(1.0)))
        else:  # (no uniform fill in f64: a constant; the kernels' work does not depend on the values)
            v = np.array([1.5], dt)
            lib._ck(lib.c.smhip_fill(C.c_int(sma.DTYPES[np.dtype(dt)]), C.c_void_p(a.ptr), v.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        red_shape = tuple(e for d, e in enumerate(shape) if d != axis)
        idx = lib.empty(red_shape, np.int64)
        red = lib.empty(red_shape, dt)
        route, launches, ori, chunk = lib.argreduce_plan("argmax", dt, list(shape), list(a.strides), axis)
        rname = {sma.ARG_ROUTE_ROW: "row", sma.ARG_ROUTE_COLUMN: "column"}.get(route & 0xff, str(route & 0xff)) + ("+split" if route & sma.ARG_SPLIT else "")
        byts = n * np.dtype(dt).itemsize
        for call in ("argmax", "+value"):

            def arg():
                if call == "argmax":
                    lib.argreduce("argmax", a, axis, out=idx)
                else:
                    lib.argreduce("argmax", a, axis, values=True, out=idx)

            def yard():
                lib.reduce("max", a, axis, out=red)

            for _ in range(args.warmup):
                arg()
                yard()
            ts, ty = [], []
            for _ in range(args.rounds):
                ts.append(timeit(arg))
                ty.append(timeit(yard))
            ms, my = statistics.median(ts), statistics.median(ty)
            ratio = my / ms
            say("%-20s %-4s %-8s %-34s %7.0f %22s %22s %7.3f %6s" % (
                label, np.dtype(dt).name[0] + str(np.dtype(dt).itemsize * 8), call, "%s %s %d %d" % (rname, ori, chunk, launches), byts / ms * 1e-3,
                "%.1f (%.1f .. %.1f)" % (ms, min(ts), max(ts)), "%.1f (%.1f .. %.1f)" % (my, min(ty), max(ty)), ratio,
                "ok" if ratio >= BAR else "UNDER"))
        del a, idx, red
        lib.pool_trim()
    say("bar: ratio >= %.2f (max time / argmax time)" % BAR)
    if args.headline:
        say(args.headline)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
