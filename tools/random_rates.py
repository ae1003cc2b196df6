"""smhip_random against smhip_fill over the same bytes, timed in the same process: every kind x dtype at 2^28 elements (1 GiB of 4-byte,
2 GiB of 8-byte results).  Both only write, so the ratio says what the Philox rounds and the maps cost on top of the store stream.
Kernel time per call from HIP events after warm-up, the two calls in alternating rounds; the median round and the spread of the
rounds (min .. max) are reported; `replay` writes the same buffer every step, `cold` rotates through disjoint buffers of >= 2.5 GiB
together.  Rates are bytes written over time, as a share of 8 TB/s; fill/new is the figure of merit (1: the draw costs nothing).

    python tools/random_rates.py [--steps K] [--rounds R] [--log2n N] [--only SUBSTRING] > profiles/random_rates.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplemath_amd as sma  # noqa: E402

PEAK_GBS = 8000.0
COLD_ROTATION_BYTES = 2560 << 20
NAMES = {sma.F32: "f32", sma.F64: "f64", sma.I32: "i32", sma.I64: "i64"}
NP = {sma.F32: np.float32, sma.F64: np.float64, sma.I32: np.int32, sma.I64: np.int64}
SIZE = {sma.F32: 4, sma.F64: 8, sma.I32: 4, sma.I64: 8}
ROWS = [("bits", sma.RANDOM_BITS, sma.I32, None), ("bits", sma.RANDOM_BITS, sma.I64, None),
        ("uniform", sma.RANDOM_UNIFORM, sma.F32, (0.0, 1.0)), ("uniform", sma.RANDOM_UNIFORM, sma.F64, (0.0, 1.0)),
        ("integers", sma.RANDOM_INTEGERS, sma.I32, (0.0, 1000.0)), ("integers", sma.RANDOM_INTEGERS, sma.I64, (0.0, 1000.0)),
        ("bernoulli", sma.RANDOM_BERNOULLI, sma.F32, (0.9, 0.0)), ("bernoulli", sma.RANDOM_BERNOULLI, sma.F64, (0.9, 0.0)),
        ("bernoulli", sma.RANDOM_BERNOULLI, sma.I32, (0.9, 0.0)), ("bernoulli", sma.RANDOM_BERNOULLI, sma.I64, (0.9, 0.0)),
        ("normal", sma.RANDOM_NORMAL, sma.F32, (0.0, 1.0)), ("normal", sma.RANDOM_NORMAL, sma.F64, (0.0, 1.0))]


class Raw:
    def __init__(self, path):
        self.c = C.CDLL(path)
        self.c.smhip_last_error.restype = C.c_char_p
        self.c.smhip_random.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]

    def ck(self, rc):
        if rc < 0:
            raise RuntimeError(self.c.smhip_last_error().decode())

    def sync(self):
        self.ck(self.c.smhip_synchronize())

    def time(self, calls, steps, warmup):
        """us per call; calls[i % len(calls)] is step i (one entry: replay; several: cold)"""
        for i in range(max(warmup, len(calls))):
            calls[i % len(calls)]()
        e0, e1, ms = C.c_void_p(0), C.c_void_p(0), C.c_float(0)
        self.ck(self.c.smhip_event_create(C.byref(e0)))
        self.ck(self.c.smhip_event_create(C.byref(e1)))
        self.sync()
        self.ck(self.c.smhip_event_record(e0))
        for i in range(steps):
            calls[i % len(calls)]()
        self.ck(self.c.smhip_event_record(e1))
        self.sync()
        self.ck(self.c.smhip_event_elapsed_ms(e0, e1, C.byref(ms)))
        self.c.smhip_event_destroy(e0)
        self.c.smhip_event_destroy(e1)
        return ms.value / steps * 1000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--only", default=None, help="substring of the row labels to run")
    args = ap.parse_args()
    lib = Raw(os.environ.get("SMHIP_LIBRARY", sma.LIB_PATH))
    n = 1 << args.log2n

    def alloc(nbytes):
        p = C.c_void_p(0)
        lib.ck(lib.c.smhip_alloc(C.byref(p), C.c_size_t(nbytes)))
        return p.value

    def random_call(kind, dtype, params, out):
        pp = (C.c_double * 2)(*params) if params is not None else None
        return lambda: lib.ck(lib.c.smhip_random(kind, dtype, out, n, 42, 0, 0, pp))

    def fill_call(dtype, out):
        v = np.array([1], dtype=NP[dtype])
        return lambda: lib.ck(lib.c.smhip_fill(C.c_int(dtype), C.c_void_p(out), v.ctypes.data_as(C.c_void_p), C.c_size_t(n)))

    print("%-22s %-6s %8s %19s %8s %19s %8s %7s %7s" % ("random, 2^%d elements" % args.log2n, "set", "new us", "(min .. max)", "fill us", "(min .. max)", "fill/new", "new", "fill"))
    print("# rates: bytes written over the median time, as a share of 8 TB/s; fill: smhip_fill of the same dtype over the same bytes")
    for name, kind, dtype, params in ROWS:
        label = "%s %s" % (name, NAMES[dtype])
        if args.only and args.only not in label:
            continue
        nbytes = n * SIZE[dtype]
        k = max(2, -(-COLD_ROTATION_BYTES // nbytes))
        bufs = [alloc(nbytes) for _ in range(k)]
        lib.sync()
        for setting in ("replay", "cold"):
            use = bufs[:1] if setting == "replay" else bufs
            cn = [random_call(kind, dtype, params, b) for b in use]
            cy = [fill_call(dtype, b) for b in use]
            tn, ty = [], []
            for _ in range(args.rounds):  # alternating: new, yardstick, new, yardstick ...
                tn.append(lib.time(cn, max(args.steps, 2 * len(cn)), args.warmup))
                ty.append(lib.time(cy, max(args.steps, 2 * len(cy)), args.warmup))
            n_us, y_us = float(np.median(tn)), float(np.median(ty))
            print("%-22s %-6s %8.1f (%7.1f ..%7.1f) %8.1f (%7.1f ..%7.1f) %8.3f %6.1f%% %6.1f%%"
                  % (label, setting, n_us, min(tn), max(tn), y_us, min(ty), max(ty), y_us / n_us, nbytes / n_us * 1e-3 / PEAK_GBS * 100,
                     nbytes / y_us * 1e-3 / PEAK_GBS * 100), flush=True)
        for p in bufs:
            lib.c.smhip_free(C.c_void_p(p))
        lib.sync()
        lib.c.smhip_pool_trim()


if __name__ == "__main__":
    main()
