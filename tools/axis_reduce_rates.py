"""Axis reductions (smhip_reduce_axes) on the issue's shape table: kernel time per call from HIP events after warm-up, as a
fraction of 8 TB/s over the algorithmic bytes (input + output).  Inputs are >= 512 MiB so that the Infinity Cache does
not flatter them.  The HBM traffic behind a row is checked with `rocprofv3 --kernel-trace --stats -- python
tools/axis_reduce_rates.py` in a run of its own.

    python tools/axis_reduce_rates.py [--steps K]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplemath_amd as sma  # noqa: E402

PEAK_GBS = 8000.0
TABLE = [  # label, shape, dtype, axes, transposed view (the operand is a.T)
    ("16384x16384 f32 axis 1 (rows)", (16384, 16384), np.float32, 1, False),
    ("16384x16384 f32 axis 0 (columns)", (16384, 16384), np.float32, 0, False),
    ("16384x16384 f32 .T axis 0", (16384, 16384), np.float32, 0, True),
    ("(2^20, 256) f32 axis 1 (short rows)", (1 << 20, 256), np.float32, 1, False),
    ("(2^26, 4) f32 axis 0 (split)", (1 << 26, 4), np.float32, 0, False),
    ("(4, 2^26) f32 axis 1 (split)", (4, 1 << 26), np.float32, 1, False),
    ("(1024,224,224,3) f32 axes 0-2", (1024, 224, 224, 3), np.float32, (0, 1, 2), False),
    ("8192x8192 f64 axis 0", (8192, 8192), np.float64, 0, False),
    ("8192x8192 f64 axis 1", (8192, 8192), np.float64, 1, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="sum,max")
    args = ap.parse_args()
    lib = sma.load()
    lib.set_device(0)

    def timeit(fn):
        for _ in range(args.warmup):
            fn()
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

    print("%-38s %-5s %-24s %8s %9s %7s" % ("shape", "kind", "route (O, R, I)", "us", "GB/s", "of 8TB/s"))
    for label, shape, dt, axes, transposed in TABLE:
        n = int(np.prod(shape))
        a = lib.empty((n,), dt)
        if dt == np.float32:
            lib._ck(lib.c.smhip_fill_uniform_f32(C.c_void_p(a.ptr), C.c_size_t(n), C.c_uint64(7), C.c_uint64(0), C.c_float(-1.0), C.c_float(1.0)))
        else:
            one = np.array([1.5], dt)
            lib._ck(lib.c.smhip_fill(C.c_int(sma.DTYPES[np.dtype(dt)]), C.c_void_p(a.ptr), one.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        st, acc = [], 1
        for d in shape[::-1]:
            st.append(acc)
            acc *= d
        st = st[::-1]
        if transposed:
            view = sma.DeviceArray(lib, a.base_ptr, dt, shape[::-1], st[::-1], 0, a._owner)
        else:
            view = sma.DeviceArray(lib, a.base_ptr, dt, shape, st, 0, a._owner)
        ax = (axes,) if isinstance(axes, int) else axes
        out_n = int(np.prod([e for d, e in enumerate(view.shape) if d not in ax]))
        out = lib.empty((max(out_n, 1),), dt)
        route, launches, ori = lib.reduce_plan("sum", dt, list(view.shape), list(view.strides), axes)
        rname = {1: "row", 2: "column", 3: "channel"}.get(route & 0xff, str(route & 0xff))
        if route & sma.ROUTE_SPLIT:
            rname += "+split"
        if route & sma.ROUTE_COPY:
            rname += "+copy"
        byts = (n + out_n) * np.dtype(dt).itemsize
        for kind in args.kinds.split(","):
            t = timeit(lambda: lib.reduce(kind, view, axes, out=out))
            gbs = byts / t * 1e-3
            print("%-38s %-5s %-24s %8.1f %9.0f %6.1f%%" % (label, kind, "%s %s" % (rname, ori), t, gbs, gbs / PEAK_GBS * 100), flush=True)
        del view, out, a
        lib.pool_trim()


if __name__ == "__main__":
    main()
