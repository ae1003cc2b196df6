"""astype (smhip_convert) against a yardstick with the same memory traffic, timed in the same process: DENSE for all 12 pairs at 2^26
and 2^28 elements against smhip_unary(NEG) on the SOURCE type over an array sized to move the same number of bytes (n * (S + D) =
2 * m * S), and ROWS / STAGED for a 4096^2 block of columns and a 4096^2 transpose against DENSE of the same pair and size.
Kernel time per call from HIP events after warm-up, the two calls in alternating rounds; the median round and the spread of the
rounds (min .. max) are reported; `replay` re-reads the same operands every step, `cold` rotates through disjoint operand sets of
>= 2.5 GiB together.  Rates are algorithmic bytes (what the route's contract says it moves) over time, as a share of 8 TB/s.

    python tools/astype_rates.py [--steps K] [--rounds R] [--only SUBSTRING] > profiles/astype_rates.txt
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


class Raw:
    def __init__(self, path):
        self.c = C.CDLL(path)
        self.c.smhip_last_error.restype = C.c_char_p

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


def i64(seq):
    return (C.c_int64 * len(seq))(*seq)


def convert_call(lib, s, d, a, shape, strides, out):
    st, sh = i64(strides), i64(shape)
    return lambda: lib.ck(lib.c.smhip_convert(C.c_int(s), C.c_int(d), C.c_void_p(a), st, sh, C.c_int(len(shape)), C.c_void_p(out)))


def neg_call(lib, dtype, a, n, out):
    st, sh = i64([1]), i64([n])
    return lambda: lib.ck(lib.c.smhip_unary(C.c_int(sma.UNARY_NEG), C.c_int(dtype), C.c_void_p(a), st, sh, C.c_int(1), C.c_void_p(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="substring of the row labels to run")
    args = ap.parse_args()
    lib = Raw(sma.LIB_PATH)
    rng = np.random.default_rng(1)
    seeds = {sma.F32: rng.uniform(-1000, 1000, 1 << 22).astype(np.float32), sma.F64: rng.uniform(-1e12, 1e12, 1 << 22),
             sma.I32: rng.integers(-10 ** 9, 10 ** 9, 1 << 22).astype(np.int32), sma.I64: rng.integers(-10 ** 15, 10 ** 15, 1 << 22)}

    def alloc(nbytes):
        p = C.c_void_p(0)
        lib.ck(lib.c.smhip_alloc(C.byref(p), C.c_size_t(nbytes)))
        return p.value

    def operand(dtype, n):  # n elements: 2^22 random values, repeated
        esz = SIZE[dtype]
        p = alloc(n * esz)
        m = min(n, seeds[dtype].size)
        lib.ck(lib.c.smhip_upload(C.c_void_p(p), seeds[dtype].ctypes.data_as(C.c_void_p), C.c_size_t(m * esz)))
        done = m
        while done < n:
            k = min(done, n - done)
            lib.ck(lib.c.smhip_copy(C.c_void_p(p + done * esz), C.c_void_p(p), C.c_size_t(k * esz)))
            done += k
        return p

    def free_all(sets):
        for s in sets:
            for p in s:
                lib.c.smhip_free(C.c_void_p(p))
        lib.sync()
        lib.c.smhip_pool_trim()

    def measure(label, ylabel, alg_bytes, new_sets, make_new, yard_sets, make_yard):
        for setting in ("replay", "cold"):
            cn = [make_new(s) for s in (new_sets[:1] if setting == "replay" else new_sets)]
            cy = [make_yard(s) for s in (yard_sets[:1] if setting == "replay" else yard_sets)]
            tn, ty = [], []
            for _ in range(args.rounds):  # alternating: new, yardstick, new, yardstick ...
                tn.append(lib.time(cn, max(args.steps, 2 * len(cn)), args.warmup))
                ty.append(lib.time(cy, max(args.steps, 2 * len(cy)), args.warmup))
            n_us, y_us = float(np.median(tn)), float(np.median(ty))
            print("%-26s %-22s %-6s %8.1f (%7.1f ..%7.1f) %8.1f (%7.1f ..%7.1f) %6.3f %6.1f%% %6.1f%%"
                  % (label, ylabel, setting, n_us, min(tn), max(tn), y_us, min(ty), max(ty), y_us / n_us, alg_bytes / n_us * 1e-3 / PEAK_GBS * 100,
                     alg_bytes / y_us * 1e-3 / PEAK_GBS * 100), flush=True)

    print("%-26s %-22s %-6s %8s %19s %8s %19s %6s %7s %7s" % ("astype", "yardstick", "set", "new us", "(min .. max)", "yard us", "(min .. max)", "y/new",
                                                              "new", "yard"))
    print("# rates: algorithmic bytes over the median time, as a share of 8 TB/s; y/new > 1: astype is the faster of the two")
    types = [sma.F32, sma.F64, sma.I32, sma.I64]
    for log2n in (26, 28):
        n = 1 << log2n
        for s in types:
            for d in types:
                label = "dense %s -> %s 2^%d" % (NAMES[s], NAMES[d], log2n)
                if s == d or (args.only and args.only not in label):
                    continue
                ss, ds = SIZE[s], SIZE[d]
                m = n * (ss + ds) // (2 * ss)  # NEG over m source elements moves the same bytes
                k = max(2, -(-COLD_ROTATION_BYTES // (n * (ss + ds))))
                new_sets = [[operand(s, n), alloc(n * ds)] for _ in range(k)]
                yard_sets = [[operand(s, m), alloc(m * ss)] for _ in range(k)]
                lib.sync()
                measure(label, "neg %s, %d el" % (NAMES[s], m), n * (ss + ds), new_sets, lambda b, s=s, d=d, n=n: convert_call(lib, s, d, b[0], [n], [1], b[1]),
                        yard_sets, lambda b, s=s, m=m: neg_call(lib, s, b[0], m, b[1]))
                free_all(new_sets + yard_sets)
    side = 4096
    for s, d in ((sma.F32, sma.F64), (sma.F64, sma.F32), (sma.F32, sma.I32), (sma.I64, sma.F32), (sma.F64, sma.I64)):
        ss, ds = SIZE[s], SIZE[d]
        n = side * side
        for route, base_elems, shape, strides, per in (("rows", 2 * n, [side, side], [2 * side, 1], ss + ds), ("staged", n, [side, side], [1, side], 3 * ss + ds)):
            label = "%s %s -> %s %d^2" % (route, NAMES[s], NAMES[d], side)
            if args.only and args.only not in label:
                continue
            k = max(2, -(-COLD_ROTATION_BYTES // (base_elems * ss + n * ds)))
            new_sets = [[operand(s, base_elems), alloc(n * ds)] for _ in range(k)]
            yard_sets = [[operand(s, n), alloc(n * ds)] for _ in range(k)]
            lib.sync()
            # rows: the block of columns [side/2, 3 side/2) of a (side, 2 side) array; staged: the transpose of a (side, side) array
            off = (side // 2) * ss if route == "rows" else 0
            measure(label, "dense, same pair", n * per, new_sets,
                    lambda b, s=s, d=d, shape=shape, strides=strides, off=off: convert_call(lib, s, d, b[0] + off, shape, strides, b[1]), yard_sets,
                    lambda b, s=s, d=d, n=n: convert_call(lib, s, d, b[0], [n], [1], b[1]))
            free_all(new_sets + yard_sets)
    print("# (the yardstick's share in the rows / staged lines is computed over the ROUTE's bytes, not DENSE's own: compare the times)")


if __name__ == "__main__":
    main()
