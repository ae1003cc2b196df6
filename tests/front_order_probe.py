"""Helper of test_front_order_gpu.py: runs the dense streaming operators at the sizes where front_order.h's walk is live and can
go wrong, and compares every result with the oracle bit for bit.  The test starts it with SMHIP_FRONT_LOG2C=1 (C = 2: groups of
G = 16 workgroups) and once more with SMHIP_PIECE_LOG2VEC=14 on top (pieces of exactly one group).
       python tests/front_order_probe.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import simplemath_amd as sma
from oracle import oracle as orc

C = 1 << int(os.environ["SMHIP_FRONT_LOG2C"])
G = 8 * C                        # workgroups per group; one workgroup = 1024 vectors
BIG = 1 << 20                    # the first size of the 1024-thread kernel
K = BIG // (G * 1024) + 1        # the first whole number of groups past it
NVEC = (BIG, BIG + 1, K * G * 1024 - 1, K * G * 1024, K * G * 1024 + 1, BIG + 3 * G * 1024 + 517)

lib = sma.load()
lib.set_device(0)
o = orc.Oracle()
rng = np.random.default_rng(20261019)
checked = 0


def fresh(dtype, n):
    """an output whose every byte is wrong until the kernel writes it"""
    return lib.to_device(np.full(n * np.dtype(dtype).itemsize, 0x7F, dtype=np.uint8).view(dtype))


def same(got, want, what):
    global checked
    g, w = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(got.view(f"u{got.itemsize}") != want.view(f"u{want.itemsize}"))
        raise SystemExit(f"{what}: {bad.size} elements differ, first at {bad[0]} (workgroup {bad[0] * got.itemsize // 16 // 1024})")
    checked += 1


for dtype in (np.float32, np.float64, np.int32, np.int64):
    W = 16 // np.dtype(dtype).itemsize
    nmax = max(NVEC) * W + W
    if np.issubdtype(dtype, np.floating):
        A, B = (rng.uniform(-100, 100, nmax).astype(dtype) for _ in range(2))
    else:
        info = np.iinfo(dtype)
        A, B = (rng.integers(info.min, info.max, nmax, dtype=dtype, endpoint=True) for _ in range(2))  # the sums wrap
    for nv in NVEC:
        for tail in (0, 1, W - 1):
            n = nv * W + tail
            a, b = np.ascontiguousarray(A[:n]), np.ascontiguousarray(B[:n])
            da, db = lib.to_device(a), lib.to_device(b)
            tag = f"{np.dtype(dtype).name} n_vec {nv} tail {tail}"
            same(lib.contiguous(sma.OP_ADD, da, db, out=fresh(dtype, n)).numpy(), o.contiguous(orc.ADD, a, b), "add " + tag)
            if dtype is not np.float32:
                continue
            s = np.float32(1.7)
            same(lib.array_scalar(sma.OP_MUL, da, s, out=fresh(dtype, n)).numpy(), o.array_scalar(orc.MUL, a, s), "a*s " + tag)
            out, sp = fresh(dtype, n), lib.alloc(8)
            lib.contiguous_sum_async(sma.OP_ADD, da, db, out, sp)
            total = lib.read_f64(sp)
            lib.free(sp)
            want_out, want_sum = o.contiguous_sum(orc.ADD, a, b)
            same(out.numpy(), want_out, "fused add+sum " + tag)
            # tests/test_gpu_parity.py: test_sum_and_fused_vs_oracle's bound (fp64 accumulation, any order)
            bound = 1e-15 * float(np.abs(want_out.astype(np.float64)).sum()) + 1e-300
            print(f"fused sum {tag}: off by {abs(total - want_sum):.3e}, bound {bound:.3e}")
            if not abs(total - want_sum) <= bound:
                raise SystemExit(f"fused sum {tag}: {total!r} against {want_sum!r}")
            checked += 1
print("front_order_probe ok", checked)
