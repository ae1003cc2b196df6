"""Functions of one argument (smhip_unary, unary chain stages) against yardsticks with the same memory traffic, timed in the
same process: each row of the table names the new call and an existing call of the PARENT commit's library (--parent-lib, a
libsmhip.so built from the parent commit; without it the yardstick comes from this library, which has the same kernels).
Kernel time per call from HIP events after warm-up, the two calls in alternating rounds, the median round reported; `replay`
re-reads the same operands every step, `cold` rotates through disjoint operand sets of >= 2.5 GiB together (bench.py --full's
two settings).  Rates are algorithmic bytes over time, as a share of 8 TB/s.

    python tools/unary_rates.py [--parent-lib PATH] [--steps K] [--rounds R]
    python tools/unary_rates.py --single     # every new row once between two marker fills: the counter runs of tools/unary_pmc.py
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
F32, F64 = sma.F32, sma.F64
DT = {F32: np.float32, F64: np.float64}
U = sma.SMHIP_OP_UNARY_BASE


class Raw:
    """The few entry points the table needs, straight through ctypes: works for a library older than this header."""

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


def unary_call(lib, fn, dtype, a, n, out):
    st, sh = i64([1]), i64([n])
    return lambda: lib.ck(lib.c.smhip_unary(C.c_int(fn), C.c_int(dtype), C.c_void_p(a), st, sh, C.c_int(1), C.c_void_p(out)))


def scalar_call(lib, op, dtype, a, n, out, value):
    v = np.array([value], DT[dtype])
    p = v.ctypes.data_as(C.c_void_p)
    return lambda _v=v: lib.ck(lib.c.smhip_array_scalar(C.c_int(op), C.c_int(dtype), C.c_void_p(a), p, C.c_size_t(n), C.c_void_p(out)))


def sqrt_t_call(lib, a, side, out):
    st, sh = i64([1, side]), i64([side, side])
    return lambda: lib.ck(lib.c.smhip_unary(C.c_int(sma.UNARY_SQRT), C.c_int(F32), C.c_void_p(a), st, sh, C.c_int(2), C.c_void_p(out)))


def copy_t_call(lib, a, side, out):
    st, sh, dst = i64([1, side]), i64([side, side]), i64([side, 1])
    return lambda: lib.ck(lib.c.smhip_copy_strided(C.c_int(F32), C.c_void_p(a), st, C.c_void_p(out), dst, sh, C.c_int(2)))


def chain_call(lib, a, col, side, out, last_op):
    """(a - col) then exp (new) or * s (yardstick)"""
    ptrs = (C.c_void_p * 3)(a, col, None)
    strides = i64([side, 1, 1, 0, 0, 0])
    scal = np.array([0, 0, 1.0009765625], np.float32)
    ops, swp, sh = (C.c_int * 2)(sma.OP_SUB, last_op), (C.c_int * 2)(0, 0), i64([side, side])
    sp = scal.ctypes.data_as(C.c_void_p)
    return lambda _k=(ptrs, strides, scal, ops, swp, sh): lib.ck(lib.c.smhip_chain(C.c_int(F32), C.c_int(3), ptrs, strides, sp, ops, swp, sh, C.c_int(2), C.c_void_p(out)))


def table():
    """(label, algorithmic bytes, operand elements per set [a, out, extra], dtype, new(lib, bufs), yardstick label, yardstick(lib, bufs))"""
    rows = []
    for log2n in (26, 28):
        n = 1 << log2n
        for dtype in (F32, F64):
            fns = [("neg", sma.UNARY_NEG), ("abs", sma.UNARY_ABS), ("sqrt", sma.UNARY_SQRT)] + ([("exp", sma.UNARY_EXP)] if dtype == F32 else [])
            esz = 4 if dtype == F32 else 8
            for name, fn in fns:
                rows.append(("%s %s 2^%d" % (name, "f32" if dtype == F32 else "f64", log2n), 2 * n * esz, [n, n], dtype,
                             lambda lib, b, fn=fn, dtype=dtype, n=n: unary_call(lib, fn, dtype, b[0], n, b[1]), "a * s",
                             lambda lib, b, dtype=dtype, n=n: scalar_call(lib, sma.OP_MUL, dtype, b[0], n, b[1], 1.0009765625)))
        rows.append(("log f32 2^%d" % log2n, 8 * n, [n, n], F32, lambda lib, b, n=n: unary_call(lib, sma.UNARY_LOG, F32, b[0], n, b[1]),
                     "pow(a, 2.5f)", lambda lib, b, n=n: scalar_call(lib, sma.OP_POW, F32, b[0], n, b[1], 2.5)))
        for name, fn in (("exp", sma.UNARY_EXP), ("log", sma.UNARY_LOG)):
            rows.append(("%s f64 2^%d" % (name, log2n), 16 * n, [n, n], F64, lambda lib, b, fn=fn, n=n: unary_call(lib, fn, F64, b[0], n, b[1]),
                         "pow(a, 2.7)", lambda lib, b, n=n: scalar_call(lib, sma.OP_POW, F64, b[0], n, b[1], 2.7)))
    side = 8192
    rows.append(("sqrt(A.T) 8192^2 f32", 8 * side * side, [side * side, side * side], F32, lambda lib, b: sqrt_t_call(lib, b[0], 8192, b[1]),
                 "copy of A.T", lambda lib, b: copy_t_call(lib, b[0], 8192, b[1])))
    for side in (4096, 8192):
        rows.append(("chain exp(a - col) %d^2 f32" % side, 8 * side * side, [side * side, side * side, side], F32,
                     lambda lib, b, side=side: chain_call(lib, b[0], b[2], side, b[1], U + sma.UNARY_EXP),
                     "chain (a - col) * s", lambda lib, b, side=side: chain_call(lib, b[0], b[2], side, b[1], sma.OP_MUL)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--only", default=None, help="substring of the row labels to run")
    args = ap.parse_args()
    new = Raw(sma.LIB_PATH)
    old = Raw(args.parent_lib) if args.parent_lib else new
    rng = np.random.default_rng(1)
    seeds = {F32: rng.uniform(0.5, 4.0, 1 << 22).astype(np.float32), F64: rng.uniform(0.5, 4.0, 1 << 22)}

    def alloc(nbytes):
        p = C.c_void_p(0)
        new.ck(new.c.smhip_alloc(C.byref(p), C.c_size_t(nbytes)))
        return p.value

    def operand(dtype, n):  # n elements: 2^22 random values in (0.5, 4), repeated
        esz = seeds[dtype].itemsize
        p = alloc(n * esz)
        m = min(n, seeds[dtype].size)
        new.ck(new.c.smhip_upload(C.c_void_p(p), seeds[dtype].ctypes.data_as(C.c_void_p), C.c_size_t(m * esz)))
        done = m
        while done < n:
            k = min(done, n - done)
            new.ck(new.c.smhip_copy(C.c_void_p(p + done * esz), C.c_void_p(p), C.c_size_t(k * esz)))
            done += k
        return p

    if not args.single:
        print("parent library: %s" % (args.parent_lib or "(none given: the yardstick runs from this library)"))
        print("%-30s %-20s %-6s %9s %9s %7s %8s" % ("new row", "yardstick", "set", "new us", "yard us", "ratio", "of 8TB/s"))
    for label, alg, elems, dtype, make_new, ylabel, make_old in table():
        if args.only and args.only not in label:
            continue
        esz = 4 if dtype == F32 else 8
        footprint = sum(elems) * esz
        if args.single:
            sets = [[operand(dtype, elems[0]), alloc(elems[1] * esz)] + [operand(dtype, e) for e in elems[2:]]]
            marker, one = alloc(1 << 16), np.array([1.0], np.float32)
            new.ck(new.c.smhip_fill(C.c_int(F32), C.c_void_p(marker), one.ctypes.data_as(C.c_void_p), C.c_size_t(1 << 14)))
            make_new(new, sets[0])()
            new.ck(new.c.smhip_fill(C.c_int(F32), C.c_void_p(marker), one.ctypes.data_as(C.c_void_p), C.c_size_t(1 << 14)))  # ... and one behind
            new.sync()
            print(label, flush=True)
            for p in sets[0] + [marker]:
                new.c.smhip_free(C.c_void_p(p))
            new.c.smhip_pool_trim()
            continue
        k = max(2, -(-COLD_ROTATION_BYTES // footprint))
        sets = [[operand(dtype, elems[0]), alloc(elems[1] * esz)] + [operand(dtype, e) for e in elems[2:]] for _ in range(k)]
        new.sync()
        for setting in ("replay", "cold"):
            use = sets[:1] if setting == "replay" else sets
            cn, co = [make_new(new, s) for s in use], [make_old(old, s) for s in use]
            steps = max(args.steps, 2 * len(use))
            tn, to = [], []
            for _ in range(args.rounds):  # alternating: new, yardstick, new, yardstick ...
                tn.append(new.time(cn, steps, args.warmup))
                to.append(old.time(co, steps, args.warmup))
            n_us, o_us = float(np.median(tn)), float(np.median(to))
            print("%-30s %-20s %-6s %9.1f %9.1f %7.3f %7.1f%%" % (label, ylabel, setting, n_us, o_us, o_us / n_us, alg / n_us * 1e-3 / PEAK_GBS * 100), flush=True)
        for s in sets:
            for p in s:
                new.c.smhip_free(C.c_void_p(p))
        new.sync()
        new.c.smhip_pool_trim()
        if old is not new:
            old.c.smhip_pool_trim()


if __name__ == "__main__":
    main()
