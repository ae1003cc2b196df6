"""The CPU model of smhip_random: the definition in include/smhip.h ("random draws") written out literally in numpy / Python-int
arithmetic.  Element i of a call is a function of (seed, stream, offset, i) alone, so any window [i0, i1) of a call comes out without
the rest: draw(..., i0=..., i1=...).

Everything is bit-exact except NORMAL, which the model evaluates in fp64 (exact octant reduction in integers, then np.cos / np.sin on
the reduced angle, sqrt(-2 log u1) in fp64) and returns as float64 whatever the dtype: the device is held to 5 ULP of it (ulp_error)."""
import numpy as np

BITS, UNIFORM, INTEGERS, BERNOULLI, NORMAL = range(5)
KINDS = {"bits": BITS, "uniform": UNIFORM, "integers": INTEGERS, "bernoulli": BERNOULLI, "normal": NORMAL}
F32, F64, I32, I64 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.int64)
PAIRS = [(BITS, I32), (BITS, I64), (UNIFORM, F32), (UNIFORM, F64), (INTEGERS, I32), (INTEGERS, I64),
         (BERNOULLI, F32), (BERNOULLI, F64), (BERNOULLI, I32), (BERNOULLI, I64), (NORMAL, F32), (NORMAL, F64)]
DEFAULT_PARAMS = {BITS: (0.0, 0.0), UNIFORM: (0.0, 1.0), INTEGERS: (-7.0, 993.0), BERNOULLI: (0.3, 0.0), NORMAL: (0.0, 1.0)}

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays holding 32-bit words; key: two Python ints -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64: no wrap
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LOW, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def block_words(seed, stream, offset, b0, b1):
    """Words of blocks b0 .. b1 - 1 of a call: shape (b1 - b0, 4), uint64 holding 32-bit values."""
    b = (np.arange(b0, b1, dtype=np.uint64) + np.uint64(offset % (1 << 64)))  # wraps like the 64-bit sum (a wrapping call is refused)
    n = b.size
    full = lambda v: np.full(n, v, dtype=np.uint64)  # noqa: E731
    w = philox4x32_10((b & LOW, b >> S32, full(stream & 0xFFFFFFFF), full((stream >> 32) & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack(w, axis=1)


def per_block(kind, dtype):
    return 2 if kind == INTEGERS else 4 if kind == BERNOULLI else 2 if np.dtype(dtype).itemsize == 8 else 4


def blocks(kind, dtype, n):
    pb = per_block(kind, dtype)
    return (n + pb - 1) // pb


def _mulhi64(x, r):
    """floor(x * r / 2^64) for uint64 x and 1 <= r <= 2^32."""
    if r == 1 << 32:
        return x >> S32
    r = np.uint64(r)
    return ((x >> S32) * r + (((x & LOW) * r) >> S32)) >> S32


def _cossin(m, bits):
    """(cos, sin) of 2 pi m / 2^bits in fp64: the octant from the top three bits, the functions on at most 1/8 turn."""
    m = m.astype(np.uint64)
    sh = np.uint64(bits - 3)
    q = (m >> sh).astype(np.int64)
    one = np.uint64(1) << sh
    f = m & (one - np.uint64(1))
    g = np.where(q & 1, one - f, f)
    a = 2.0 * np.pi * (g.astype(np.float64) / float(1 << bits))
    C, S = np.cos(a), np.sin(a)
    swap, cneg, sneg = ((q + 1) & 2) != 0, ((q + 2) & 4) != 0, q >= 4
    c, s = np.where(swap, S, C), np.where(swap, C, S)
    return np.where(cneg, -c, c), np.where(sneg, -s, s)


def _radius(k, bits):
    u1 = (k.astype(np.float64) + 1.0) / float(1 << bits)  # k < 2^53: exact
    return np.sqrt(-2.0 * np.log(u1))


def draw(kind, dtype, seed, stream, offset, n, params=None, i0=0, i1=None):
    """Elements i0 .. i1 - 1 of smhip_random(kind, dtype, out, n, seed, stream, offset, params).  NORMAL comes back as float64."""
    dtype = np.dtype(dtype)
    kind = KINDS[kind] if isinstance(kind, str) else kind
    assert (kind, dtype) in PAIRS, (kind, dtype)
    i1 = n if i1 is None else i1
    assert 0 <= i0 <= i1 <= n
    pa, pb_ = DEFAULT_PARAMS[kind] if params is None else params
    pb = per_block(kind, dtype)
    b0, b1 = i0 // pb, (i1 + pb - 1) // pb
    w = block_words(seed, stream, offset, b0, b1)
    x = w[:, 0::2] | (w[:, 1::2] << S32)  # the two 64-bit draws of a block
    wide = dtype.itemsize == 8
    if kind == BITS:
        v = x.view(np.int64) if wide else w.astype(np.uint32).view(np.int32)
    elif kind == UNIFORM:
        if wide:
            lo, span = np.float64(pa), np.float64(pb_) - np.float64(pa)
            u = (x >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)
        else:
            lo, span = np.float32(pa), np.float32(pb_) - np.float32(pa)
            u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        t = u * span
        v = lo + t
        assert v.dtype == dtype
    elif kind == INTEGERS:
        lo, r = int(pa), int(pb_) - int(pa)
        assert 1 <= r <= 1 << 32
        v = (_mulhi64(x, r).astype(np.int64) + np.int64(lo)).astype(dtype)
    elif kind == BERNOULLI:
        thr = int(np.floor(np.float64(pa) * 2.0 ** 32))
        v = (w < np.uint64(thr)).astype(dtype)
    else:
        if wide:
            r = _radius(x[:, 0] >> np.uint64(11), 53)
            c, s = _cossin(x[:, 1] >> np.uint64(11), 53)
            z = np.stack([r * c, r * s], axis=1)
        else:
            r = _radius(w[:, 0::2] >> np.uint64(8), 24)
            c, s = _cossin(w[:, 1::2] >> np.uint64(8), 24)
            z = np.stack([r[:, 0] * c[:, 0], r[:, 0] * s[:, 0], r[:, 1] * c[:, 1], r[:, 1] * s[:, 1]], axis=1)
        v = np.float64(pa) + np.float64(pb_) * z
    return np.ascontiguousarray(v.reshape(-1)[i0 - b0 * pb:i1 - b0 * pb])


def ulp_error(got, want, dtype):
    """|got - want| in spacings of `dtype` at want, elementwise (want: float64 from the model).  Where want is 0, got must be 0."""
    dtype = np.dtype(dtype)
    want = np.asarray(want, dtype=np.float64)
    ulp = np.spacing(np.abs(want.astype(dtype))).astype(np.float64)
    return np.abs(np.asarray(got).astype(np.float64) - want) / ulp


NORMAL_ULPS = 5  # two factors within 2^-23 relative each and one product rounding of 2^-24: 2.5 * 2^-23 relative
