"""simplemath_amd -- MI355X (gfx950) implementation of simpleMath's element_wise_op hot path.

The product is `libsmhip.so` (HIP kernels behind the C ABI of include/smhip.h) plus the
header-only C++20 host side in include/ (sm.h, SMArray.h, ...).  This Python package is
only the thin ctypes binding the tests and bench.py drive the C ABI through -- the same
entry points the C++ headers call.  There is no CPU fallback anywhere in it: if the
library or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import sys

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB_PATH = os.path.join(PKG, "lib", "libsmhip.so")
HEADER = os.path.join(ROOT, "include", "smhip.h")

OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_POW, OP_LEFT = range(6)
OPS = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL, "div": OP_DIV, "pow": OP_POW, "left": OP_LEFT}
F32, F64, I32, I64 = range(4)
DTYPES = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32, np.dtype(np.int64): I64}
# smhip_dot also takes the generic dot_product<T>'s other integer element types (smhip.h: SMHIP_I8 ... SMHIP_U64)
I8, U8, I16, U16, U32, U64 = range(4, 10)
DOT_DTYPES = {**DTYPES, np.dtype(np.int8): I8, np.dtype(np.uint8): U8, np.dtype(np.int16): I16, np.dtype(np.uint16): U16,
              np.dtype(np.uint32): U32, np.dtype(np.uint64): U64}
MAX_NDIM = 6

REDUCE_SUM, REDUCE_MEAN, REDUCE_MAX, REDUCE_MIN = range(4)
UNARY_NEG, UNARY_ABS, UNARY_SQRT, UNARY_EXP, UNARY_LOG = range(5)  # smhip_unary_fn
UNARY_FNS = {"neg": UNARY_NEG, "abs": UNARY_ABS, "sqrt": UNARY_SQRT, "exp": UNARY_EXP, "log": UNARY_LOG}
SMHIP_OP_UNARY_BASE = 16  # a chain stage without an operand: ops[k] = SMHIP_OP_UNARY_BASE + fn
REDUCE_KINDS = {"sum": REDUCE_SUM, "mean": REDUCE_MEAN, "max": REDUCE_MAX, "min": REDUCE_MIN}
# smhip_reduce_plan's route word: a kernel id in the low byte, flags above it
ROUTE_NONE, ROUTE_ROW, ROUTE_COLUMN, ROUTE_CHANNEL, ROUTE_FILL, ROUTE_GATHER = range(6)
ROUTE_SPLIT, ROUTE_COPY, ROUTE_PASSES = 0x100, 0x200, 0x400
SCAN_SUM, SCAN_PROD, SCAN_MAX, SCAN_MIN = range(4)  # smhip_scan_kind
SCAN_KINDS = {"cumsum": SCAN_SUM, "cumprod": SCAN_PROD, "cummax": SCAN_MAX, "cummin": SCAN_MIN}
# smhip_scan_plan's route word: a kernel id in the low byte, flags above it
SCAN_ROUTE_NONE, SCAN_ROUTE_COPYONLY, SCAN_ROUTE_ROW, SCAN_ROUTE_COLUMN = range(4)
SCAN_SPLIT, SCAN_COPY = 0x100, 0x200
ARG_MAX, ARG_MIN = range(2)  # smhip_arg_kind
ARG_KINDS = {"argmax": ARG_MAX, "argmin": ARG_MIN}
# smhip_argreduce_plan's route word: a kernel id in the low byte, flags above it
ARG_ROUTE_NONE, ARG_ROUTE_ROW, ARG_ROUTE_COLUMN = range(3)
ARG_SPLIT, ARG_COPY = 0x100, 0x200
SORT_ASCENDING, SORT_DESCENDING = range(2)  # smhip_sort_order
# smhip_sort_plan's route word: a kernel id in the low byte, flags above it
SORT_ROUTE_NONE, SORT_ROUTE_COPYONLY, SORT_ROUTE_ROW = range(3)
SORT_MERGE, SORT_COPY = 0x100, 0x200
# smhip_topk_plan's route word: a kernel id in the low byte, flags above it
TOPK_ROUTE_NONE, TOPK_ROUTE_COPYONLY, TOPK_ROUTE_ROW, TOPK_ROUTE_SORT = range(4)
TOPK_TILED, TOPK_COPY = 0x100, 0x200
TOPK_RANKED = 128  # SMHIP_TOPK_RANKED: the longest line that is ranked, whatever k is
# smhip_quantile_method, and smhip_quantile_plan's route word: a kernel id in the low byte, flags above it
QUANTILE_LINEAR, QUANTILE_LOWER, QUANTILE_HIGHER, QUANTILE_NEAREST, QUANTILE_MIDPOINT = range(5)
QUANTILE_METHODS = {"linear": QUANTILE_LINEAR, "lower": QUANTILE_LOWER, "higher": QUANTILE_HIGHER, "nearest": QUANTILE_NEAREST, "midpoint": QUANTILE_MIDPOINT}
QUANTILE_ROUTE_NONE, QUANTILE_ROUTE_COPYONLY, QUANTILE_ROUTE_ROW, QUANTILE_ROUTE_SORT = range(4)
QUANTILE_STREAM, QUANTILE_COPY = 0x100, 0x200
# smhip_softmax_kind, and smhip_softmax_plan's route word: a kernel id in the low byte, flags above it
SOFTMAX, LOG_SOFTMAX, LOGSUMEXP = range(3)
SOFTMAX_KINDS = {"softmax": SOFTMAX, "log_softmax": LOG_SOFTMAX, "logsumexp": LOGSUMEXP}
SOFTMAX_ROUTE_NONE, SOFTMAX_ROUTE_ROW, SOFTMAX_ROUTE_COLUMN, SOFTMAX_ROUTE_FILL = range(4)
SOFTMAX_SPLIT, SOFTMAX_COPY = 0x100, 0x200
# smhip_moment_kind, and the route word of smhip_moments_plan / smhip_standardize_plan: a kernel id in the low byte, flags above it
MOMENT_VAR, MOMENT_STD = range(2)
MOMENT_KINDS = {"var": MOMENT_VAR, "std": MOMENT_STD}
MOMENTS_ROUTE_NONE, MOMENTS_ROUTE_ROW, MOMENTS_ROUTE_COLUMN, MOMENTS_ROUTE_CHANNEL, MOMENTS_ROUTE_UNIT = range(5)
MOMENTS_SPLIT, MOMENTS_COPY = 0x100, 0x200
INDEX_CHECKED, INDEX_CLIP, INDEX_WRAP = range(3)  # smhip_index_mode
INDEX_MODES = {"checked": INDEX_CHECKED, "raise": INDEX_CHECKED, "clip": INDEX_CLIP, "wrap": INDEX_WRAP}
# smhip_take_plan's route word: a kernel id in the low byte, the flag above it
TAKE_ROUTE_NONE, TAKE_ROUTE_LINE, TAKE_ROUTE_ROWS, TAKE_ROUTE_DIRECT = range(4)
TAKE_COPY = 0x100
SCATTER_PUT, SCATTER_ADD = range(2)  # smhip_scatter_kind
SCATTER_UNIQUE = 1                   # smhip_scatter_axis's flag: no two entries of a line name the same position
# smhip_scatter_plan's route word: a kernel id in the low byte, the flag above it
SCATTER_ROUTE_NONE, SCATTER_ROUTE_DIRECT, SCATTER_ROUTE_ROWS, SCATTER_ROUTE_SORTED, SCATTER_ROUTE_SORTED_ROWS = range(5)
SCATTER_COPY = 0x100
SIDE_LEFT, SIDE_RIGHT = range(2)  # smhip_side
SIDES = {"left": SIDE_LEFT, "right": SIDE_RIGHT}
COUNT_SEARCHSORTED, COUNT_BINCOUNT, COUNT_HISTOGRAM = range(3)  # smhip_count_op
COUNT_OPS = {"searchsorted": COUNT_SEARCHSORTED, "bincount": COUNT_BINCOUNT, "histogram": COUNT_HISTOGRAM}
HISTOGRAM_UNIFORM = 1  # smhip_histogram's flag: the table is the uniform one of (bins, lo, hi)
# smhip_count_plan's route word: a route in the low byte, the flag above it
COUNT_ROUTE_NONE, COUNT_ROUTE_LDS, COUNT_ROUTE_GLOBAL = range(3)
COUNT_COPY = 0x100
CMP_NONZERO, CMP_EQ, CMP_NE, CMP_LT, CMP_LE, CMP_GT, CMP_GE = range(7)  # smhip_cmp
CMPS = {"nonzero": CMP_NONZERO, "eq": CMP_EQ, "ne": CMP_NE, "lt": CMP_LT, "le": CMP_LE, "gt": CMP_GT, "ge": CMP_GE,
        "==": CMP_EQ, "!=": CMP_NE, "<": CMP_LT, "<=": CMP_LE, ">": CMP_GT, ">=": CMP_GE}
SELECT_INDEX, SELECT_COORDS, SELECT_VALUES, SELECT_COUNT, SELECT_WHERE = range(5)  # smhip_select_what (the last two: smhip_select_plan only)
SELECT_OPS = {"index": SELECT_INDEX, "coords": SELECT_COORDS, "values": SELECT_VALUES, "count": SELECT_COUNT, "where": SELECT_WHERE}
# smhip_select_plan's route word: a route in the low byte, the flag above it
SELECT_ROUTE_NONE, SELECT_ROUTE_ONE, SELECT_ROUTE_TILES, SELECT_ROUTE_DENSE = range(4)
SELECT_COPY = 0x100
RUNS_NAN_DISTINCT = 1  # smhip_runs' flag: a NaN is a run of its own (equal_nan=False)
RUNS_VALUES, RUNS_INDEX, RUNS_COUNTS, RUNS_INVERSE = 1, 2, 4, 8  # smhip_runs_plan's `outputs`
RUNS_ROUTE_NONE, RUNS_ROUTE_ONE, RUNS_ROUTE_TILES = range(3)
CONVERT_ROUTE_NONE, CONVERT_ROUTE_DENSE, CONVERT_ROUTE_ROWS, CONVERT_ROUTE_STAGED, CONVERT_ROUTE_COPY = range(5)  # smhip_convert_route
RANDOM_BITS, RANDOM_UNIFORM, RANDOM_INTEGERS, RANDOM_BERNOULLI, RANDOM_NORMAL = range(5)  # smhip_random_kind
RANDOM_KINDS = {"bits": RANDOM_BITS, "uniform": RANDOM_UNIFORM, "integers": RANDOM_INTEGERS, "bernoulli": RANDOM_BERNOULLI, "normal": RANDOM_NORMAL}

ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_BROADCAST = -1, -2, -3, -4, -5


class SmhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"smhip error {code}: {msg}")
        self.code = code


def declared_symbols():
    """Every function name include/smhip.h declares."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smhip_[a-z0-9_]+)\s*\(", text)))


def _i64(seq):
    return (C.c_int64 * max(len(seq), 1))(*[int(x) for x in seq])


class DeviceArray:
    """A (possibly strided) view on device memory: what sm::SMArray<T> holds host-side."""

    def __init__(self, lib, base_ptr, dtype, shape, strides, offset=0, owner=None):
        self.lib, self.base_ptr, self.dtype = lib, base_ptr, np.dtype(dtype)
        self.shape, self.strides, self.offset = tuple(int(s) for s in shape), tuple(int(s) for s in strides), int(offset)
        self._owner = owner if owner is not None else _Owner(lib, base_ptr)

    @property
    def ptr(self):
        # `lib.to_device(x).ptr` hands out the address of a block that returns to the pool the moment the expression ends
        # (two of round 3's red runs were that).  A temporary has no reference beyond the ones this call itself holds:
        # the evaluation stack, `self`, and getrefcount's argument.
        if sys.getrefcount(self) <= 3 and sys.getrefcount(self._owner) <= 2:  # (a temporary VIEW of a live array is fine: the owner lives on)
            raise RuntimeError("DeviceArray.ptr on a temporary: its memory goes back to the pool when this expression ends -- "
                               "keep the array in a variable for as long as the pointer is in use")
        return self.base_ptr + self.offset * self.dtype.itemsize

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1

    @property
    def ndim(self):
        return len(self.shape)

    def is_dense(self):
        exp = 1
        for d, s in zip(self.shape[::-1], self.strides[::-1]):
            if s != exp:
                return False
            exp *= d
        return True

    def view_like(self, np_view, np_base):
        """The same view numpy made on the host base, on the device base."""
        if np_view.size and not np.shares_memory(np_view, np_base):  # a view of ANOTHER array would turn into a wild device pointer
            raise ValueError("view_like: np_view is not a view of np_base")
        off = (np_view.__array_interface__["data"][0] - np_base.__array_interface__["data"][0]) // self.dtype.itemsize
        return DeviceArray(self.lib, self.base_ptr, self.dtype, np_view.shape,
                           [s // self.dtype.itemsize for s in np_view.strides], off, self._owner)

    def numpy(self):
        assert self.is_dense(), "download a dense array (views alias their parent)"
        out = np.empty(self.shape, dtype=self.dtype)
        self.lib.download(out, self.ptr)
        return out


class _Owner:
    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def __del__(self):
        try:
            self.lib.free(self.ptr)
        except Exception:
            pass


class Smhip:
    """ctypes face of include/smhip.h."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: build it with `python -m simplemath_amd.build` "
                                    "(there is no CPU fallback)")
        self.path = path
        self.c = C.CDLL(path)
        c = self.c
        c.smhip_version.restype = C.c_char_p
        c.smhip_last_error.restype = C.c_char_p
        for name in declared_symbols():
            fn = getattr(c, name)  # AttributeError here = header/library mismatch
            if name not in ("smhip_version", "smhip_last_error"):
                fn.restype = C.c_int
        c.smhip_fill_uniform_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_float, C.c_float]
        c.smhip_random.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]
        c.smhip_random_blocks.argtypes = [C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint64)]

    # -- plumbing ---------------------------------------------------------
    def _ck(self, rc):
        if rc < 0:
            raise SmhipError(rc, self.c.smhip_last_error().decode())
        return rc

    def version(self):
        return self.c.smhip_version().decode()

    def device_count(self):
        n = C.c_int(0)
        self._ck(self.c.smhip_device_count(C.byref(n)))
        return n.value

    def set_device(self, d):
        self._ck(self.c.smhip_set_device(C.c_int(d)))

    def set_stream(self, stream_ptr):
        self._ck(self.c.smhip_set_stream(C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._ck(self.c.smhip_synchronize())

    def alloc(self, nbytes):
        p = C.c_void_p(0)
        self._ck(self.c.smhip_alloc(C.byref(p), C.c_size_t(nbytes)))
        return p.value

    def free(self, ptr):
        self._ck(self.c.smhip_free(C.c_void_p(ptr)))

    def pool_trim(self):
        self._ck(self.c.smhip_pool_trim())

    def pool_stats(self):
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._ck(self.c.smhip_pool_stats(C.byref(a), C.byref(b)))
        return a.value, b.value

    def upload(self, ptr, host: np.ndarray):
        host = np.ascontiguousarray(host)
        self._ck(self.c.smhip_upload(C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)))

    def copy(self, dst_ptr, src_ptr, nbytes):
        """Device-to-device copy on the library's stream."""
        self._ck(self.c.smhip_copy(C.c_void_p(dst_ptr), C.c_void_p(src_ptr), C.c_size_t(nbytes)))

    def download(self, host: np.ndarray, ptr):
        assert host.flags.c_contiguous
        self._ck(self.c.smhip_download(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(host.nbytes)))

    # -- arrays -----------------------------------------------------------
    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        n = int(np.prod(shape, dtype=np.int64))
        ptr = self.alloc(max(n, 1) * dtype.itemsize)
        strides, acc = [], 1
        for d in shape[::-1]:
            strides.append(acc)
            acc *= d
        return DeviceArray(self, ptr, dtype, shape, strides[::-1])

    def to_device(self, host: np.ndarray):
        host = np.ascontiguousarray(host)
        d = self.empty(host.shape if host.ndim else (1,), host.dtype)
        self.upload(d.ptr, host)
        return d

    def full(self, shape, value, dtype):
        d = self.empty(shape, dtype)
        v = np.array([value], dtype=dtype)
        self._ck(self.c.smhip_fill(C.c_int(DTYPES[d.dtype]), C.c_void_p(d.ptr), v.ctypes.data_as(C.c_void_p), C.c_size_t(d.size)))
        return d

    def uniform_f32(self, n, seed, lo, hi, first=0):
        d = self.empty((n,), np.float32)
        self._ck(self.c.smhip_fill_uniform_f32(C.c_void_p(d.ptr), n, seed, first, lo, hi))
        return d

    # -- shape layer --------------------------------------------------------
    def broadcast(self, shape1, strides1, shape2, strides2):
        nd = max(len(shape1), len(shape2))
        rs, s1, s2 = _i64([0] * nd), _i64([0] * nd), _i64([0] * nd)
        tot = C.c_int64(0)
        rc = self.c.smhip_broadcast(C.c_int(len(shape1)), _i64(shape1), _i64(strides1), C.c_int(len(shape2)),
                                    _i64(shape2), _i64(strides2), rs, s1, s2, C.byref(tot))
        if rc == ERR_BROADCAST:
            return None
        self._ck(rc)
        return list(rs[:nd]), list(s1[:nd]), list(s2[:nd]), tot.value

    def is_contiguous(self, shape, strides):
        return bool(self.c.smhip_is_contiguous(C.c_int(len(shape)), _i64(shape), _i64(strides)))

    def register_op(self, hip_expression: str) -> int:
        """User-defined Op: a HIP expression in `a` and `b`; returns the op id to pass as `op`."""
        oid = C.c_int(0)
        self._ck(self.c.smhip_register_op(hip_expression.encode(), C.byref(oid)))
        return oid.value

    # -- hot path -------------------------------------------------------------
    def elementwise_raw(self, op, dtype, a_ptr, sa, b_ptr, sb, shape, out_ptr):
        self._ck(self.c.smhip_elementwise(C.c_int(op), C.c_int(DTYPES[np.dtype(dtype)]), C.c_void_p(a_ptr), _i64(sa),
                                          C.c_void_p(b_ptr), _i64(sb), _i64(shape), C.c_int(len(shape)), C.c_void_p(out_ptr)))

    def binary(self, op, a: DeviceArray, b: DeviceArray, out: DeviceArray | None = None):
        """a op b with broadcasting: what SMArray::operator+ does (SMArray.h:217-225)."""
        assert a.dtype == b.dtype
        res = self.broadcast(a.shape, a.strides, b.shape, b.strides)
        if res is None:
            raise RuntimeError("Cannot broadcast shapes: incompatible dimensions")
        shape, sa, sb, _ = res
        if out is None:
            out = self.empty(shape, a.dtype)
        self.elementwise_raw(op, a.dtype, a.ptr, sa, b.ptr, sb, shape, out.ptr)
        return out

    def binary_inline(self, op, a, b):
        """a op b where a host numpy array (<= 1 KiB) rides in the kernel's argument block instead of being uploaded
        (smhip_elementwise_inline); a, b: numpy arrays (inline) or DeviceArrays; a numpy scalar is an inline operand of one element."""
        def side(x):
            if isinstance(x, DeviceArray):
                return x.shape, x.strides, C.c_void_p(x.ptr), 0, x.dtype, None
            h = np.ascontiguousarray(x)
            if h.ndim == 0:
                h = h.reshape(1)
            return h.shape, [st // h.itemsize for st in h.strides], h.ctypes.data_as(C.c_void_p), h.nbytes, h.dtype, h
        sha, sta, pa, na, dta, keep_a = side(a)
        shb, stb, pb, nb, dtb, keep_b = side(b)
        assert dta == dtb
        res = self.broadcast(sha, sta, shb, stb)
        if res is None:
            raise RuntimeError("Cannot broadcast shapes: incompatible dimensions")
        shape, sa, sb, _ = res
        out = self.empty(shape, dta)
        self._ck(self.c.smhip_elementwise_inline(C.c_int(op), C.c_int(DTYPES[np.dtype(dta)]), pa, C.c_size_t(na), _i64(sa), pb, C.c_size_t(nb),
                                                 _i64(sb), _i64(shape), C.c_int(len(shape)), C.c_void_p(out.ptr)))
        return out

    def assign(self, dst: DeviceArray, src: DeviceArray):
        """dst[...] = src, element by element (src broadcast to dst's shape): SMArray::operator=(SMArray&&), SMArray.h:89-97."""
        assert dst.dtype == src.dtype
        res = self.broadcast(dst.shape, dst.strides, src.shape, src.strides)
        if res is None or tuple(res[0]) != tuple(dst.shape):
            raise RuntimeError("Shape mismatch in assignment")
        shape, sd, ss, _ = res
        self._ck(self.c.smhip_copy_strided(C.c_int(DTYPES[dst.dtype]), C.c_void_p(src.ptr), _i64(ss), C.c_void_p(dst.ptr), _i64(sd),
                                           _i64(shape), C.c_int(len(shape))))

    def contiguous(self, op, a: DeviceArray, b: DeviceArray, out: DeviceArray | None = None):
        assert a.dtype == b.dtype and a.size == b.size
        if out is None:
            out = self.empty(a.shape, a.dtype)
        self._ck(self.c.smhip_contiguous(C.c_int(op), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), C.c_void_p(b.ptr),
                                         C.c_void_p(out.ptr), C.c_size_t(a.size)))
        return out

    def array_scalar(self, op, a: DeviceArray, value, out: DeviceArray | None = None):
        if out is None:
            out = self.empty(a.shape, a.dtype)
        v = np.array([value], dtype=a.dtype)
        self._ck(self.c.smhip_array_scalar(C.c_int(op), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr),
                                           v.ctypes.data_as(C.c_void_p), C.c_size_t(a.size), C.c_void_p(out.ptr)))
        return out

    def fused(self, op1, op2, a: DeviceArray, b: DeviceArray, c, out: DeviceArray | None = None):
        """(a op1 b) op2 c in one pass; c a DeviceArray or a scalar."""
        if out is None:
            out = self.empty(a.shape, a.dtype)
        if isinstance(c, DeviceArray):
            cp, sp = C.c_void_p(c.ptr), C.c_void_p(0)
        else:
            v = np.array([c], dtype=a.dtype)
            cp, sp = C.c_void_p(0), v.ctypes.data_as(C.c_void_p)
        self._ck(self.c.smhip_fused_contiguous(C.c_int(op1), C.c_int(op2), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr),
                                               C.c_void_p(b.ptr), cp, sp, C.c_void_p(out.ptr), C.c_size_t(a.size)))
        return out

    def unary(self, fn, a: DeviceArray, out: DeviceArray | None = None):
        """out = fn(a), fn one of "neg", "abs", "sqrt", "exp", "log" or the smhip_unary_fn value; `a` any view (read in place by
        neg / abs / sqrt, copied dense first by exp / log) -> a new dense DeviceArray, or into `out`, which must be a dense array
        of a's dtype and element count (its shape is not changed); `out` may be `a` itself when `a` is dense (in place)."""
        fn = UNARY_FNS[fn] if isinstance(fn, str) else int(fn)
        if out is None:
            out = self.empty(a.shape, a.dtype)
        elif out.dtype != a.dtype or out.size != a.size or not out.is_dense():
            raise ValueError(f"unary: out must be a dense {a.dtype} array of {a.size} elements (shape {tuple(a.shape)}); "
                             f"got {out.dtype} {out.shape} dense={out.is_dense()}")
        self._ck(self.c.smhip_unary(C.c_int(fn), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(a.strides), _i64(a.shape),
                                    C.c_int(a.ndim), C.c_void_p(out.ptr)))
        return out

    def unary_raw(self, fn, dtype, a_ptr, strides, shape, out_ptr):
        """smhip_unary with every argument as given (argument-validation tests)."""
        return self.c.smhip_unary(C.c_int(fn), C.c_int(dtype), C.c_void_p(a_ptr), _i64(strides) if strides is not None else None,
                                  _i64(shape) if shape is not None else None, C.c_int(len(shape) if shape is not None else 0),
                                  C.c_void_p(out_ptr))

    # -- changing the element type ------------------------------------------------------
    @staticmethod
    def _convert_dtype(dtype, who):
        try:
            dt = np.dtype(dtype)
        except TypeError as e:
            raise TypeError(f"{who}: {dtype!r} is not an element type") from e
        if dt not in DTYPES:
            raise TypeError(f"{who}: element type {dt} is not one of float32, float64, int32, int64")
        return dt

    def astype(self, a: DeviceArray, dtype, out: DeviceArray | None = None):
        """np.ndarray.astype on the device between float32, float64, int32 and int64 (smhip_convert; smhip.h has the rules: float to
        integer is saturating truncation, NaN gives 0).  `a` any view -> a new dense DeviceArray of a's shape, or into `out`, which
        must be a dense array of `dtype` and a's shape and must not overlap `a`.  The same dtype gives a dense copy."""
        dt = self._convert_dtype(dtype, "astype")
        self._convert_dtype(a.dtype, "astype")
        if out is None:
            out = self.empty(a.shape, dt)
        elif out.dtype != dt:
            raise TypeError(f"astype: out is {out.dtype}, the result is {dt}")
        elif tuple(out.shape) != tuple(a.shape) or not out.is_dense():
            raise ValueError(f"astype: out must be a dense array of shape {tuple(a.shape)}; got {tuple(out.shape)} dense={out.is_dense()}")
        self._ck(self.c.smhip_convert(C.c_int(DTYPES[a.dtype]), C.c_int(DTYPES[dt]), C.c_void_p(a.ptr), _i64(a.strides), _i64(a.shape),
                                      C.c_int(a.ndim), C.c_void_p(out.ptr)))
        return out

    def convert_raw(self, src_dtype, dst_dtype, a_ptr, strides, shape, out_ptr):
        """smhip_convert with every argument as given (argument-validation tests)."""
        return self.c.smhip_convert(C.c_int(src_dtype), C.c_int(dst_dtype), C.c_void_p(a_ptr), _i64(strides) if strides is not None else None,
                                    _i64(shape) if shape is not None else None, C.c_int(len(shape) if shape is not None else 0),
                                    C.c_void_p(out_ptr))

    def convert_plan(self, src_dtype, dst_dtype, shape, strides, ndim=None):
        """smhip_convert_plan (host only): (route, launches, bytes moved) for converting a view of these shape and strides (elements)."""
        src_dtype = DTYPES[self._convert_dtype(src_dtype, "convert_plan")] if not isinstance(src_dtype, int) else src_dtype
        dst_dtype = DTYPES[self._convert_dtype(dst_dtype, "convert_plan")] if not isinstance(dst_dtype, int) else dst_dtype
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        route, launches, moved = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._ck(self.c.smhip_convert_plan(C.c_int(src_dtype), C.c_int(dst_dtype), arr(shape), arr(strides), C.c_int(ndim), C.byref(route),
                                           C.byref(launches), C.byref(moved)))
        return route.value, launches.value, moved.value

    # -- random draws ---------------------------------------------------------------------
    def _random_pair(self, kind, dtype, who):
        """(kind id, dtype) of a draw; TypeError for an element type the kind is not defined for."""
        kind = RANDOM_KINDS[kind] if isinstance(kind, str) else int(kind)
        dt = self._convert_dtype(dtype, who)
        floats = dt.kind == "f"
        if (kind in (RANDOM_UNIFORM, RANDOM_NORMAL) and not floats) or (kind in (RANDOM_BITS, RANDOM_INTEGERS) and floats):
            raise TypeError(f"{who}: not defined for element type {dt}")
        return kind, dt

    def random_blocks(self, kind, dtype, n):
        """smhip_random_blocks (host only): the Philox blocks a call of n elements consumes."""
        kind, dt = self._random_pair(kind, dtype, "random_blocks")
        blocks = C.c_uint64(0)
        self._ck(self.c.smhip_random_blocks(kind, DTYPES[dt], int(n), C.byref(blocks)))
        return blocks.value

    def random_raw(self, kind, dtype, out_ptr, n, seed, stream, offset, params):
        """smhip_random with every argument as given (argument-validation tests); params: a pair of floats or None."""
        pp = (C.c_double * 2)(*params) if params is not None else None
        return self.c.smhip_random(int(kind), int(dtype), C.c_void_p(out_ptr), int(n), int(seed), int(stream), int(offset), pp)

    def generator(self, seed, stream=0):
        """A counter-based generator (sm::Generator): uniform, normal, integers, bernoulli, bits, permutation, shuffle; each call
        advances its position by the blocks it consumed, so a program's draws are reproducible."""
        return Generator(self, seed, stream)

    @staticmethod
    def _stage(st):
        """(op, x, swapped) of a chain stage; a one-element stage -- ("exp",) or (SMHIP_OP_UNARY_BASE + fn,) -- is a function of
        one argument applied to the chain's value: no operand (x = None)."""
        if len(st) == 1:
            op = st[0]
            return (SMHIP_OP_UNARY_BASE + UNARY_FNS[op] if isinstance(op, str) else int(op), None, False)
        return (OPS[st[0]] if isinstance(st[0], str) else int(st[0]), st[1], bool(len(st) > 2 and st[2]))

    def chain_call(self, first: DeviceArray, *stages, out: DeviceArray | None = None):
        """(callable, out): the prepared smhip_chain call for `chain(first, *stages)` -- timing loops call it without
        paying the argument marshalling again."""
        dt = first.dtype
        shape = list(first.shape)
        stages = [self._stage(st) for st in stages]
        for st in stages:
            x = st[1]
            if isinstance(x, DeviceArray):
                assert x.dtype == dt
                res = self.broadcast(shape, [0] * len(shape), x.shape, x.strides)
                if res is None:
                    raise RuntimeError("Cannot broadcast shapes: incompatible dimensions")
                shape = res[0]
        nd = len(shape)
        operands = [first] + [st[1] for st in stages]
        strides, ptrs, scal = [], [], np.zeros(len(operands), dtype=dt)
        for k, x in enumerate(operands):
            if isinstance(x, DeviceArray):
                res = self.broadcast(shape, [0] * nd, x.shape, x.strides)
                strides += list(res[2])
                ptrs.append(x.ptr)
            else:
                strides += [0] * nd
                ptrs.append(None)
                if x is not None:
                    scal[k] = x
        if out is None:
            out = self.empty(shape, dt)
        ops = (C.c_int * len(stages))(*[int(st[0]) for st in stages])
        swp = (C.c_int * len(stages))(*[1 if len(st) > 2 and st[2] else 0 for st in stages])
        args = (C.c_int(DTYPES[dt]), C.c_int(len(operands)), (C.c_void_p * len(operands))(*ptrs), _i64(strides),
                scal.ctypes.data_as(C.c_void_p), ops, swp, _i64(shape), C.c_int(nd), C.c_void_p(out.ptr))
        keep = (operands, scal, out)  # the arrays stay alive as long as the callable does
        fn = self.c.smhip_chain

        def call(_keep=keep):
            rc = fn(*args)
            if rc < 0:
                self._ck(rc)
        return call, out

    def chain_sum_call(self, first: DeviceArray, *stages):
        """(callable -> float): the prepared smhip_chain_sum call for the sum of `chain(first, *stages)`'s value, which is not written."""
        dt = first.dtype
        shape = list(first.shape)
        stages = [self._stage(st) for st in stages]
        for st in stages:
            x = st[1]
            if isinstance(x, DeviceArray):
                assert x.dtype == dt
                res = self.broadcast(shape, [0] * len(shape), x.shape, x.strides)
                if res is None:
                    raise RuntimeError("Cannot broadcast shapes: incompatible dimensions")
                shape = res[0]
        nd = len(shape)
        operands = [first] + [st[1] for st in stages]
        strides, ptrs, scal = [], [], np.zeros(len(operands), dtype=dt)
        for k, x in enumerate(operands):
            if isinstance(x, DeviceArray):
                res = self.broadcast(shape, [0] * nd, x.shape, x.strides)
                strides += list(res[2])
                ptrs.append(x.ptr)
            else:
                strides += [0] * nd
                ptrs.append(None)
                if x is not None:
                    scal[k] = x
        ops = (C.c_int * len(stages))(*[int(st[0]) for st in stages])
        swp = (C.c_int * len(stages))(*[1 if len(st) > 2 and st[2] else 0 for st in stages])
        result = C.c_double(0.0)
        args = (C.c_int(DTYPES[dt]), C.c_int(len(operands)), (C.c_void_p * len(operands))(*ptrs), _i64(strides),
                scal.ctypes.data_as(C.c_void_p), ops, swp, _i64(shape), C.c_int(nd), C.byref(result))
        keep = (operands, scal)
        fn = self.c.smhip_chain_sum

        def call(_keep=keep):
            self._ck(fn(*args))
            return result.value
        return call

    def chain_sum(self, first: DeviceArray, *stages):
        """sum(chain(first, *stages)) without writing the chain's value (smhip_chain_sum): fp64 / wrapping 64-bit accumulation."""
        return self.chain_sum_call(first, *stages)()

    def chain(self, first: DeviceArray, *stages, out: DeviceArray | None = None):
        """An operator chain in as few passes as possible (smhip_chain): r = first; then for each stage (op, x) -- or
        (op, x, True) for the swapped form x op r -- r = r op x with NumPy broadcasting; x a DeviceArray or a scalar.
        What SMArray's operators queue when a temporary feeds the next operator of the same expression."""
        call, out = self.chain_call(first, *stages, out=out)
        call()
        return out

    def fused_expr(self, expression: str, *arrays: DeviceArray, scalars=(), out: DeviceArray | None = None):
        """out = EXPR(a0, a1, ..., s0, ...) in one pass over dense, equal-sized operands (smhip_fused_expr)."""
        a0 = arrays[0]
        assert all(a.dtype == a0.dtype and a.size == a0.size and a.is_dense() for a in arrays)
        if out is None:
            out = self.empty(a0.shape, a0.dtype)
        ptrs = (C.c_void_p * len(arrays))(*[a.ptr for a in arrays])
        sc = np.array(list(scalars), dtype=a0.dtype)
        self._ck(self.c.smhip_fused_expr(expression.encode(), C.c_int(DTYPES[a0.dtype]), ptrs, C.c_int(len(arrays)),
                                         sc.ctypes.data_as(C.c_void_p) if len(sc) else None, C.c_int(len(sc)), C.c_void_p(out.ptr),
                                         C.c_size_t(a0.size)))
        return out

    def fused_expr_bcast(self, expression: str, *arrays: DeviceArray, scalars=(), out: DeviceArray | None = None):
        """out = EXPR(a0, a1, ..., s0, ...) in one pass over operands that broadcast against each other (smhip_fused_expr_bcast)."""
        a0 = arrays[0]
        shape = list(a0.shape)
        for a in arrays[1:]:
            assert a.dtype == a0.dtype
            res = self.broadcast(shape, [0] * len(shape), a.shape, a.strides)
            if res is None:
                raise RuntimeError("Cannot broadcast shapes: incompatible dimensions")
            shape = res[0]
        nd = len(shape)
        strides = []
        for a in arrays:
            strides += list(self.broadcast(shape, [0] * nd, a.shape, a.strides)[2])
        if out is None:
            out = self.empty(shape, a0.dtype)
        ptrs = (C.c_void_p * len(arrays))(*[a.ptr for a in arrays])
        sc = np.array(list(scalars), dtype=a0.dtype)
        self._ck(self.c.smhip_fused_expr_bcast(expression.encode(), C.c_int(DTYPES[a0.dtype]), ptrs, _i64(strides), C.c_int(len(arrays)),
                                               sc.ctypes.data_as(C.c_void_p) if len(sc) else None, C.c_int(len(sc)), _i64(shape), C.c_int(nd),
                                               C.c_void_p(out.ptr)))
        return out

    def fused_expr_sum(self, expression: str, *arrays: DeviceArray, scalars=(), store=False):
        """sum_i EXPR(a0[i], ...) in one pass; store=True also returns the elementwise result.  Blocks for the value."""
        a0 = arrays[0]
        assert all(a.dtype == a0.dtype and a.size == a0.size and a.is_dense() for a in arrays)
        out = self.empty(a0.shape, a0.dtype) if store else None
        ptrs = (C.c_void_p * len(arrays))(*[a.ptr for a in arrays])
        sc = np.array(list(scalars), dtype=a0.dtype)
        sp = self.alloc(8)
        try:
            self._ck(self.c.smhip_fused_expr_sum_async(expression.encode(), C.c_int(DTYPES[a0.dtype]), ptrs, C.c_int(len(arrays)),
                                                       sc.ctypes.data_as(C.c_void_p) if len(sc) else None, C.c_int(len(sc)),
                                                       C.c_void_p(out.ptr) if store else None, C.c_size_t(a0.size), C.c_void_p(sp)))
            total = self.read_f64(sp)
        finally:
            self.free(sp)
        return (total, out) if store else total

    def dot(self, a: DeviceArray, b: DeviceArray):
        out = np.zeros(1, dtype=a.dtype)
        self._ck(self.c.smhip_dot(C.c_int(DOT_DTYPES[a.dtype]), C.c_void_p(a.ptr), C.c_void_p(b.ptr), C.c_size_t(a.size),
                                  out.ctypes.data_as(C.c_void_p)))
        return out[0]

    def dot_c64(self, a_ptr, b_ptr, n):
        out = np.zeros(2, dtype=np.float64)
        self._ck(self.c.smhip_dot_c64(C.c_void_p(a_ptr), C.c_void_p(b_ptr), C.c_size_t(n), out.ctypes.data_as(C.c_void_p)))
        return complex(out[0], out[1])

    def dot_c32(self, a_ptr, b_ptr, n):
        out = np.zeros(2, dtype=np.float32)
        self._ck(self.c.smhip_dot_c32(C.c_void_p(a_ptr), C.c_void_p(b_ptr), C.c_size_t(n), out.ctypes.data_as(C.c_void_p)))
        return np.complex64(complex(out[0], out[1]))

    @staticmethod
    def _axes(ndim, axis):
        """NumPy's `axis` (an int, a tuple, or None for all) as a sorted tuple of axes; a bad or repeated axis raises."""
        axes = tuple(range(ndim)) if axis is None else (axis,) if isinstance(axis, (int, np.integer)) else tuple(axis)
        norm = []
        for ax in axes:
            ax = int(ax)
            if not -ndim <= ax < ndim:
                raise ValueError(f"axis {ax} is out of bounds for an array of dimension {ndim}")
            norm.append(ax % ndim)
        if len(set(norm)) != len(norm):
            raise ValueError(f"repeated axis in {axis}")
        return tuple(sorted(norm))

    def reduce(self, kind, a: DeviceArray, axis=None, keepdims=False, out: DeviceArray | None = None):
        """np.sum / np.mean / np.max / np.min of `a` (any view) over `axis` (int or tuple) -> a new dense DeviceArray, or into
        `out`, which must be a dense array of a's dtype with as many elements as the result (its shape is not changed).
        Reducing every axis without keepdims gives shape (1,) (a DeviceArray has no 0-d form)."""
        kind = REDUCE_KINDS[kind] if isinstance(kind, str) else int(kind)
        axes = self._axes(a.ndim, axis)
        mask = sum(1 << d for d in axes)
        if keepdims:
            shape = tuple(1 if d in axes else n for d, n in enumerate(a.shape))
        else:
            shape = tuple(n for d, n in enumerate(a.shape) if d not in axes) or (1,)
        if out is None:
            out = self.empty(shape, a.dtype)
        elif out.dtype != a.dtype or out.size != int(np.prod(shape, dtype=np.int64)) or not out.is_dense():
            raise ValueError(f"reduce: out must be a dense {a.dtype} array of {int(np.prod(shape, dtype=np.int64))} elements "
                             f"(shape {shape}); got {out.dtype} {out.shape} dense={out.is_dense()}")
        self._ck(self.c.smhip_reduce_axes(C.c_int(kind), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(a.shape), _i64(a.strides),
                                          C.c_int(a.ndim), C.c_uint32(mask), C.c_void_p(out.ptr)))
        return out

    def reduce_raw(self, kind, dtype, a_ptr, shape, strides, mask, out_ptr):
        """smhip_reduce_axes with every argument as given (argument-validation tests)."""
        return self.c.smhip_reduce_axes(C.c_int(kind), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                        _i64(strides) if strides is not None else None, C.c_int(len(shape) if shape is not None else 0),
                                        C.c_uint32(mask), C.c_void_p(out_ptr))

    def reduce_plan(self, kind, dtype, shape, strides, axis):
        """smhip_reduce_plan (host only): (route word, launches, (O, R, I)) for a call on shape / strides (elements) over `axis`."""
        kind = REDUCE_KINDS[kind] if isinstance(kind, str) else int(kind)
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        axes = self._axes(len(shape), axis)
        route, launches, ori = C.c_int(0), C.c_int(0), (C.c_int64 * 3)()
        self._ck(self.c.smhip_reduce_plan(C.c_int(kind), C.c_int(dtype), _i64(shape), _i64(strides), C.c_int(len(shape)),
                                          C.c_uint32(sum(1 << d for d in axes)), C.byref(route), C.byref(launches), ori))
        return route.value, launches.value, tuple(int(x) for x in ori)

    def scan(self, kind, a: DeviceArray, axis=None, out: DeviceArray | None = None):
        """np.cumsum / np.cumprod / np.maximum.accumulate / np.minimum.accumulate of `a` (any view) along `axis` ("cumsum",
        "cumprod", "cummax", "cummin" or the smhip_scan_kind value) -> a new dense DeviceArray of a's shape, or into `out`,
        which must be a dense array of a's dtype and element count (its shape is not changed); `out` may be `a` itself when
        `a` is dense (in place).  axis=None scans the elements in row-major order and gives shape (a.size,)."""
        kind = SCAN_KINDS[kind] if isinstance(kind, str) else int(kind)
        if axis is None:
            if not a.is_dense():  # the row-major order of a view: its dense copy
                dense = self.empty(a.shape, a.dtype)
                self.assign(dense, a)
                a = dense
            shape, strides, axis, result_shape = (a.size,), (1,), 0, (a.size,)
        else:
            (axis,) = self._axes(a.ndim, int(axis))
            shape, strides, result_shape = a.shape, a.strides, a.shape
        if out is None:
            out = self.empty(result_shape, a.dtype)
        elif out.dtype != a.dtype or out.size != a.size or not out.is_dense():
            raise ValueError(f"scan: out must be a dense {a.dtype} array of {a.size} elements (shape {tuple(result_shape)}); "
                             f"got {out.dtype} {out.shape} dense={out.is_dense()}")
        self._ck(self.c.smhip_scan_axis(C.c_int(kind), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(shape), _i64(strides),
                                        C.c_int(len(shape)), C.c_int(axis), C.c_void_p(out.ptr)))
        return out

    def scan_raw(self, kind, dtype, a_ptr, shape, strides, axis, out_ptr, ndim=None):
        """smhip_scan_axis with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        return self.c.smhip_scan_axis(C.c_int(kind), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                      _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_int(axis), C.c_void_p(out_ptr))

    def scan_plan(self, kind, dtype, shape, strides, axis):
        """smhip_scan_plan (host only): (route word, launches, (O, R, I), chunk length) for a call on shape / strides (elements)."""
        kind = SCAN_KINDS[kind] if isinstance(kind, str) else int(kind)
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        route, launches, ori, chunk = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), C.c_int64(0)
        self._ck(self.c.smhip_scan_plan(C.c_int(kind), C.c_int(dtype), _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(int(axis)),
                                        C.byref(route), C.byref(launches), ori, C.byref(chunk)))
        return route.value, launches.value, tuple(int(x) for x in ori), chunk.value

    def argreduce(self, kind, a: DeviceArray, axis=None, keepdims=False, values=False, out: DeviceArray | None = None):
        """np.argmax / np.argmin of `a` (any view) along `axis` ("argmax", "argmin" or the smhip_arg_kind value) -> a new dense
        int64 DeviceArray of positions along the axis, or into `out`, which must be a dense int64 array with as many elements
        as the result (its shape is not changed).  values=True returns (values, indices) from the same single pass, the values
        being exactly the elements at those positions.  axis=None gives the row-major index of the whole view, shape (1,) (a
        DeviceArray has no 0-d form); a view that is not dense is copied dense first."""
        kind = ARG_KINDS[kind] if isinstance(kind, str) else int(kind)
        if a.dtype not in DTYPES:
            raise ValueError(f"argreduce: dtype {a.dtype} (f32, f64, i32 and i64 only)")
        if axis is None:
            if not a.is_dense():  # the row-major order of a view: its dense copy
                dense = self.empty(a.shape, a.dtype)
                self.assign(dense, a)
                a = dense
            shape, strides, axis = (a.size,), (1,), 0
            result_shape = (1,) * a.ndim if keepdims else (1,)
        else:
            (axis,) = self._axes(a.ndim, int(axis))
            shape, strides = a.shape, a.strides
            if keepdims:
                result_shape = tuple(1 if d == axis else n for d, n in enumerate(a.shape))
            else:
                result_shape = tuple(n for d, n in enumerate(a.shape) if d != axis) or (1,)
        count = int(np.prod(result_shape, dtype=np.int64))
        if out is None:
            out = self.empty(result_shape, np.int64)
        elif out.dtype != np.dtype(np.int64) or out.size != count or not out.is_dense():
            raise ValueError(f"argreduce: out must be a dense int64 array of {count} elements (shape {tuple(result_shape)}); "
                             f"got {out.dtype} {out.shape} dense={out.is_dense()}")
        vals = self.empty(result_shape, a.dtype) if values else None
        self._ck(self.c.smhip_argreduce_axis(C.c_int(kind), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(shape), _i64(strides),
                                             C.c_int(len(shape)), C.c_int(axis), C.c_void_p(out.ptr), C.c_void_p(vals.ptr if values else 0)))
        return (vals, out) if values else out

    def argreduce_raw(self, kind, dtype, a_ptr, shape, strides, axis, index_ptr, value_ptr=0, ndim=None):
        """smhip_argreduce_axis with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        return self.c.smhip_argreduce_axis(C.c_int(kind), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                           _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_int(axis),
                                           C.c_void_p(index_ptr), C.c_void_p(value_ptr))

    def argreduce_plan(self, kind, dtype, shape, strides, axis):
        """smhip_argreduce_plan (host only): (route word, launches, (O, R, I), chunk length) for a call on shape / strides (elements)."""
        kind = ARG_KINDS[kind] if isinstance(kind, str) else int(kind)
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        route, launches, ori, chunk = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), C.c_int64(0)
        self._ck(self.c.smhip_argreduce_plan(C.c_int(kind), C.c_int(dtype), _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(int(axis)),
                                             C.byref(route), C.byref(launches), ori, C.byref(chunk)))
        return route.value, launches.value, tuple(int(x) for x in ori), chunk.value

    def sort(self, a: DeviceArray, axis=-1, descending=False, indices=False, out: DeviceArray | None = None):
        """np.sort(a, axis, kind="stable") of `a` (any view) -> a new dense DeviceArray of a's shape, or into `out`, which must be a
        dense array of a's dtype and element count (its shape is not changed); `out` may be `a` itself when `a` is dense (in
        place).  descending=True puts NaNs, then the larger values first, ties still in the order of their positions (not the
        ascending result reversed).  indices=True returns (values, indices) from the same call, the int64 positions along the
        axis that np.argsort(kind="stable") gives.  axis=None sorts the row-major flattening and gives shape (a.size,)."""
        return self._sort(a, axis, descending, True, indices, out, None)

    def argsort(self, a: DeviceArray, axis=-1, descending=False, out: DeviceArray | None = None):
        """np.argsort(a, axis, kind="stable") -> a new dense int64 DeviceArray of a's shape (or into `out`, a dense int64 array
        with as many elements): the positions along the axis in sorted order; `descending` and axis=None as in sort()."""
        return self._sort(a, axis, descending, False, True, None, out)

    def _sort(self, a, axis, descending, want_values, want_indices, out, index_out):
        if a.dtype not in DTYPES:
            raise ValueError(f"sort: dtype {a.dtype} (f32, f64, i32 and i64 only)")
        if axis is None:
            if not a.is_dense():  # the row-major order of a view: its dense copy
                if out is a:
                    raise ValueError("sort: out=a (in place) needs a dense array")
                dense = self.empty(a.shape, a.dtype)
                self.assign(dense, a)
                a = dense
            shape, strides, axis, result_shape = (a.size,), (1,), 0, (a.size,)
        else:
            (axis,) = self._axes(a.ndim, int(axis))
            shape, strides, result_shape = a.shape, a.strides, a.shape
        vals = idx = None
        if want_values:
            if out is None:
                vals = self.empty(result_shape, a.dtype)
            elif out is a and not a.is_dense():
                raise ValueError("sort: out=a (in place) needs a dense array")
            elif out.dtype != a.dtype or out.size != a.size or not out.is_dense():
                raise ValueError(f"sort: out must be a dense {a.dtype} array of {a.size} elements (shape {tuple(result_shape)}); "
                                 f"got {out.dtype} {out.shape} dense={out.is_dense()}")
            else:
                vals = out
        if want_indices:
            if index_out is None:
                idx = self.empty(result_shape, np.int64)
            elif index_out.dtype != np.dtype(np.int64) or index_out.size != a.size or not index_out.is_dense():
                raise ValueError(f"argsort: out must be a dense int64 array of {a.size} elements (shape {tuple(result_shape)}); "
                                 f"got {index_out.dtype} {index_out.shape} dense={index_out.is_dense()}")
            else:
                idx = index_out
        self._ck(self.c.smhip_sort_axis(C.c_int(SORT_DESCENDING if descending else SORT_ASCENDING), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr),
                                        _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(axis),
                                        C.c_void_p(vals.ptr if vals is not None else 0), C.c_void_p(idx.ptr if idx is not None else 0)))
        return (vals, idx) if want_values and want_indices else vals if want_values else idx

    def sort_raw(self, order, dtype, a_ptr, shape, strides, axis, values_ptr=0, index_ptr=0, ndim=None):
        """smhip_sort_axis with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        return self.c.smhip_sort_axis(C.c_int(order), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                      _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_int(axis),
                                      C.c_void_p(values_ptr), C.c_void_p(index_ptr))

    def sort_plan(self, dtype, shape, strides, axis, descending=False):
        """smhip_sort_plan (host only): (route word, launches, (O, R, I), K or R) for a call on shape / strides (elements)."""
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        route, launches, ori, chunk = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), C.c_int64(0)
        self._ck(self.c.smhip_sort_plan(C.c_int(SORT_DESCENDING if descending else SORT_ASCENDING), C.c_int(dtype), _i64(shape), _i64(strides),
                                        C.c_int(len(shape)), C.c_int(int(axis)), C.byref(route), C.byref(launches), ori, C.byref(chunk)))
        return route.value, launches.value, tuple(int(x) for x in ori), chunk.value

    def topk(self, a: DeviceArray, k, axis=-1, largest=True, out: DeviceArray | None = None, index_out: DeviceArray | None = None):
        """The first k along `axis` of sort(a, axis, descending=largest, indices=True), without the sort -> (values, indices): new
        dense DeviceArrays of a's shape with shape[axis] replaced by k (or `out` / `index_out`, dense arrays of a's dtype / int64 with
        as many elements, never the operand).  largest=True: NaNs, then the larger values first; largest=False: the smaller values
        first, NaNs last; equal elements in rising position.  `a` is any view; axis=None takes the row-major flattening and gives
        shape (k,).  ValueError for a dtype outside f32, f64, i32 and i64, k outside 0..shape[axis], or a bad out / index_out."""
        if a.dtype not in DTYPES:
            raise ValueError(f"topk: dtype {a.dtype} (f32, f64, i32 and i64 only)")
        k = int(k)
        if axis is None:
            if not a.is_dense():  # the row-major order of a view: its dense copy
                dense = self.empty(a.shape, a.dtype)
                self.assign(dense, a)
                a = dense
            shape, strides, axis = (a.size,), (1,), 0
        else:
            (axis,) = self._axes(a.ndim, int(axis))
            shape, strides = a.shape, a.strides
        if k < 0 or k > shape[axis]:
            raise ValueError(f"topk: k {k} outside 0..{shape[axis]}")
        result_shape = tuple(shape[:axis]) + (k,) + tuple(shape[axis + 1:])
        n = int(np.prod(result_shape, dtype=np.int64))
        for given, dtype, name in ((out, a.dtype, "out"), (index_out, np.dtype(np.int64), "index_out")):
            if given is not None and (given.dtype != dtype or given.size != n or not given.is_dense()):
                raise ValueError(f"topk: {name} must be a dense {dtype} array of {n} elements (shape {result_shape}); "
                                 f"got {given.dtype} {given.shape} dense={given.is_dense()}")
        vals = out if out is not None else self.empty(result_shape, a.dtype)
        idx = index_out if index_out is not None else self.empty(result_shape, np.int64)
        self._ck(self.c.smhip_topk_axis(C.c_int(SORT_DESCENDING if largest else SORT_ASCENDING), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr),
                                        _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(axis), C.c_int64(k),
                                        C.c_void_p(vals.ptr), C.c_void_p(idx.ptr)))
        return vals, idx

    def topk_raw(self, order, dtype, a_ptr, shape, strides, axis, k, values_ptr=0, index_ptr=0, ndim=None):
        """smhip_topk_axis with every argument as given (argument-validation tests, one output alone); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        return self.c.smhip_topk_axis(C.c_int(order), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                      _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_int(axis), C.c_int64(k),
                                      C.c_void_p(values_ptr), C.c_void_p(index_ptr))

    def topk_plan(self, dtype, shape, strides, axis, k, largest=True):
        """smhip_topk_plan (host only): (route word, launches, (O, R, I), (L, kmax, selection levels)) for a call on shape / strides (elements)."""
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        route, launches, ori, info = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), (C.c_int64 * 3)()
        self._ck(self.c.smhip_topk_plan(C.c_int(SORT_DESCENDING if largest else SORT_ASCENDING), C.c_int(dtype), _i64(shape), _i64(strides),
                                        C.c_int(len(shape)), C.c_int(int(axis)), C.c_int64(int(k)), C.byref(route), C.byref(launches), ori, info))
        return route.value, launches.value, tuple(int(x) for x in ori), tuple(int(x) for x in info)

    def quantile(self, a: DeviceArray, q, axis=-1, method="linear", keepdims=False, out: DeviceArray | None = None):
        """np.quantile(a, q, axis, method=method) of `a` (any view, float32 or float64) along `axis`, one call -> a new dense DeviceArray
        over the other axes (keepdims=True: with extent 1 along the axis), with a leading axis of len(q) when q is a sequence; or into
        `out`, a dense array of a's dtype with as many elements, never the operand.  axis=None runs over the row-major flattening (a
        scalar q then gives shape (1,)).  method: linear, lower, higher, nearest or midpoint.  A line that holds a NaN gives NaN; every
        zero is read as +0.  TypeError for an integer dtype (astype first); ValueError for a bad axis, method, q outside [0, 1] or NaN,
        an empty q, an empty axis with a result that is not empty, or a wrong out."""
        return self._quantile("quantile", a, q, axis, method, keepdims, out, 1.0)

    def percentile(self, a: DeviceArray, p, axis=-1, method="linear", keepdims=False, out: DeviceArray | None = None):
        """quantile(a, p / 100, ...): the division is one fp64 operation per entry."""
        return self._quantile("percentile", a, p, axis, method, keepdims, out, 100.0)

    def median(self, a: DeviceArray, axis=-1, keepdims=False, out: DeviceArray | None = None):
        """quantile(a, 0.5, axis): the middle element, or the mean of the two middle ones formed as the interpolation forms it."""
        return self._quantile("median", a, 0.5, axis, "linear", keepdims, out, 1.0)

    def _quantile(self, name, a, q, axis, method, keepdims, out, scale):
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"{name}: dtype {a.dtype} (float32 and float64 only: astype first)")
        if method not in QUANTILE_METHODS:
            raise ValueError(f"{name}: method {method!r} (one of {', '.join(QUANTILE_METHODS)})")
        scalar = np.ndim(q) == 0
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
        if qs.ndim != 1 or qs.size == 0:
            raise ValueError(f"{name}: q must be a number or a non-empty 1-D sequence")
        qs = qs / scale if scale != 1.0 else qs
        if not bool(np.all((qs >= 0.0) & (qs <= 1.0))):
            raise ValueError(f"{name}: q outside [0, {scale:g}] or NaN")
        if axis is None:
            if not a.is_dense():  # the row-major order of a view: its dense copy
                dense = self.empty(a.shape, a.dtype)
                self.assign(dense, a)
                a = dense
            shape, strides, axis = (a.size,), (1,), 0
            kept = (1,) * a.ndim if keepdims else ()
        else:
            (axis,) = self._axes(a.ndim, int(axis))
            shape, strides = tuple(a.shape), tuple(a.strides)
            kept = shape[:axis] + ((1,) if keepdims else ()) + shape[axis + 1:]
        result_shape = (() if scalar else (qs.size,)) + kept or (1,)
        count = int(np.prod(result_shape, dtype=np.int64))
        if count and shape[axis] == 0:
            raise ValueError(f"{name}: an empty axis with a result that is not empty")
        if out is None:
            out = self.empty(result_shape, a.dtype)
        elif out.dtype != a.dtype or out.size != count or not out.is_dense():
            raise ValueError(f"{name}: out must be a dense {a.dtype} array of {count} elements (shape {result_shape}); "
                             f"got {out.dtype} {out.shape} dense={out.is_dense()}")
        try:
            self._ck(self.c.smhip_quantile_axis(C.c_int(QUANTILE_METHODS[method]), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(shape), _i64(strides),
                                                C.c_int(len(shape)), C.c_int(axis), (C.c_double * qs.size)(*qs.tolist()), C.c_int64(qs.size), C.c_void_p(out.ptr)))
        except SmhipError as e:
            if e.code == ERR_INVALID:
                raise ValueError(str(e)) from None
            raise
        return out

    def quantile_raw(self, method, dtype, a_ptr, shape, strides, axis, q, out_ptr=0, ndim=None, nq=None):
        """smhip_quantile_axis with every argument as given (argument-validation tests); ndim defaults to len(shape), nq to len(q)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        if nq is None:
            nq = len(q) if q is not None else 0
        return self.c.smhip_quantile_axis(C.c_int(method), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                          _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_int(axis),
                                          (C.c_double * max(len(q), 1))(*q) if q is not None else None, C.c_int64(nq), C.c_void_p(out_ptr))

    def quantile_plan(self, dtype, shape, strides, axis, q, method="linear"):
        """smhip_quantile_plan (host only): (route word, launches, (O, R, I), (L, Qmax, reads)) for a call on shape / strides (elements)."""
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        method = QUANTILE_METHODS[method] if isinstance(method, str) else int(method)
        qs = [float(x) for x in np.atleast_1d(q)]
        route, launches, ori, info = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), (C.c_int64 * 3)()
        self._ck(self.c.smhip_quantile_plan(C.c_int(method), C.c_int(dtype), _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(int(axis)),
                                            (C.c_double * len(qs))(*qs), C.c_int64(len(qs)), C.byref(route), C.byref(launches), ori, info))
        return route.value, launches.value, tuple(int(x) for x in ori), tuple(int(x) for x in info)

    def softmax(self, a: DeviceArray, axis=-1, out: DeviceArray | None = None):
        """softmax of `a` (any view, float32 or float64) along `axis`, one fused call -> a new dense DeviceArray of a's shape, or into
        `out`, a dense array of a's shape and dtype; `out` may be `a` itself when `a` is dense (in place).  axis=None takes the row-major
        flattening and gives shape (a.size,).  TypeError for an integer dtype, ValueError for a bad axis or out."""
        return self._softmax(SOFTMAX, "softmax", a, axis, False, out)

    def log_softmax(self, a: DeviceArray, axis=-1, out: DeviceArray | None = None):
        """log(softmax(a, axis)) without forming the softmax: (x - max) - log(sum(exp(x - max))), rounded once; arguments as softmax()."""
        return self._softmax(LOG_SOFTMAX, "log_softmax", a, axis, False, out)

    def logsumexp(self, a: DeviceArray, axis=-1, keepdims=False, out: DeviceArray | None = None):
        """log(sum(exp(a), axis)) -> a new dense DeviceArray over the other axes (keepdims=True: with extent 1 along the axis), or into
        `out`, a dense array of that shape and a's dtype, never the operand.  axis=None runs over the row-major flattening: shape (1,)."""
        return self._softmax(LOGSUMEXP, "logsumexp", a, axis, keepdims, out)

    def _softmax(self, kind, name, a, axis, keepdims, out):
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"{name}: dtype {a.dtype} (float32 and float64 only)")
        if axis is None:
            if not a.is_dense():  # the row-major order of a view: its dense copy
                if out is a:
                    raise ValueError(f"{name}: out=a (in place) needs a dense array")
                dense = self.empty(a.shape, a.dtype)
                self.assign(dense, a)
                a = dense
            shape, strides, axis = (a.size,), (1,), 0
        else:
            (axis,) = self._axes(a.ndim, int(axis))
            shape, strides = tuple(a.shape), tuple(a.strides)
        if kind == LOGSUMEXP:
            result_shape = shape[:axis] + ((1,) if keepdims else ()) + shape[axis + 1:]
            if not result_shape:
                result_shape = (1,)
        else:
            result_shape = shape
        if out is None:
            out = self.empty(result_shape, a.dtype)
        elif out is a and kind != LOGSUMEXP:
            if not a.is_dense():
                raise ValueError(f"{name}: out=a (in place) needs a dense array")
        elif out.dtype != a.dtype or tuple(out.shape) != tuple(result_shape) or not out.is_dense():
            raise ValueError(f"{name}: out must be a dense {a.dtype} array of shape {tuple(result_shape)}; "
                             f"got {out.dtype} {tuple(out.shape)} dense={out.is_dense()}")
        self._ck(self.c.smhip_softmax_axis(C.c_int(kind), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(shape), _i64(strides), C.c_int(len(shape)),
                                           C.c_int(axis), C.c_void_p(out.ptr)))
        return out

    def softmax_raw(self, kind, dtype, a_ptr, shape, strides, axis, out_ptr=0, ndim=None):
        """smhip_softmax_axis with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        return self.c.smhip_softmax_axis(C.c_int(kind), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                         _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_int(axis), C.c_void_p(out_ptr))

    def softmax_plan(self, kind, dtype, shape, strides, axis):
        """smhip_softmax_plan (host only): (route word, launches, (O, R, I), (L, reads, levels)) for a call on shape / strides (elements)."""
        kind = SOFTMAX_KINDS[kind] if isinstance(kind, str) else int(kind)
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        route, launches, ori, info = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), (C.c_int64 * 3)()
        self._ck(self.c.smhip_softmax_plan(C.c_int(kind), C.c_int(dtype), _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(int(axis)),
                                           C.byref(route), C.byref(launches), ori, info))
        return route.value, launches.value, tuple(int(x) for x in ori), tuple(int(x) for x in info)

    def var(self, a: DeviceArray, axis=None, ddof=0, keepdims=False, out: DeviceArray | None = None):
        """np.var(a, axis, ddof=ddof) of `a` (any view, float32 or float64) over `axis` (int, tuple, or None for all): the centred second
        moment in fp64, rounded once -> a new dense DeviceArray, or into `out`, a dense array of a's dtype with as many elements as the
        result.  Reducing every axis without keepdims gives shape (1,).  TypeError for an integer dtype; ValueError for a bad or repeated
        axis, ddof < 0, N - ddof <= 0 or a wrong out."""
        return self._moments(MOMENT_VAR, "var", a, axis, ddof, keepdims, out, False)

    def std(self, a: DeviceArray, axis=None, ddof=0, keepdims=False, out: DeviceArray | None = None):
        """np.std(a, axis, ddof=ddof): the fp64 square root of var()'s fp64 quotient, rounded once; arguments as var()."""
        return self._moments(MOMENT_STD, "std", a, axis, ddof, keepdims, out, False)

    def var_mean(self, a: DeviceArray, axis=None, ddof=0, keepdims=False, out: DeviceArray | None = None):
        """(var, mean) from one call; the mean's bytes are reduce("mean", ...)'s.  `out` receives the variance."""
        return self._moments(MOMENT_VAR, "var_mean", a, axis, ddof, keepdims, out, True)

    def _moments(self, kind, name, a, axis, ddof, keepdims, out, with_mean):
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"{name}: dtype {a.dtype} (float32 and float64 only)")
        axes = self._axes(a.ndim, axis)
        ddof = int(ddof)
        if ddof < 0:
            raise ValueError(f"{name}: ddof {ddof} is negative")
        n = int(np.prod([a.shape[d] for d in axes], dtype=np.int64))
        if keepdims:
            shape = tuple(1 if d in axes else m for d, m in enumerate(a.shape))
        else:
            shape = tuple(m for d, m in enumerate(a.shape) if d not in axes) or (1,)
        count = int(np.prod(shape, dtype=np.int64))
        if count and n - ddof <= 0:
            raise ValueError(f"{name}: N - ddof = {n} - {ddof} is not positive")
        if out is None:
            out = self.empty(shape, a.dtype)
        elif out.dtype != a.dtype or out.size != count or not out.is_dense():
            raise ValueError(f"{name}: out must be a dense {a.dtype} array of {count} elements (shape {shape}); "
                             f"got {out.dtype} {out.shape} dense={out.is_dense()}")
        mean = self.empty(shape, a.dtype) if with_mean else None
        try:
            self._ck(self.c.smhip_moments_axes(C.c_int(kind), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(a.shape), _i64(a.strides), C.c_int(a.ndim),
                                               C.c_uint32(sum(1 << d for d in axes)), C.c_int64(ddof), C.c_void_p(out.ptr),
                                               C.c_void_p(mean.ptr if with_mean else 0)))
        except SmhipError as e:
            if e.code == ERR_INVALID:
                raise ValueError(str(e)) from None
            raise
        return (out, mean) if with_mean else out

    def standardize(self, a: DeviceArray, axis=-1, eps=0.0, ddof=0, out: DeviceArray | None = None):
        """(a - mean) / sqrt(var + eps) along `axis`, statistics and quotient in fp64, rounded once -> a new dense DeviceArray of a's
        shape, or into `out`, a dense array of a's shape and dtype; `out` may be `a` itself when `a` is dense (in place).  axis=None takes
        the row-major flattening and gives shape (a.size,).  TypeError for an integer dtype; ValueError for a bad axis, a negative, NaN
        or infinite eps, ddof < 0, N - ddof <= 0 or a wrong out."""
        name = "standardize"
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"{name}: dtype {a.dtype} (float32 and float64 only)")
        eps, ddof = float(eps), int(ddof)
        if not (eps >= 0.0) or eps == float("inf"):
            raise ValueError(f"{name}: eps {eps} is negative, NaN or infinite")
        if ddof < 0:
            raise ValueError(f"{name}: ddof {ddof} is negative")
        if axis is None:
            if not a.is_dense():  # the row-major order of a view: its dense copy
                if out is a:
                    raise ValueError(f"{name}: out=a (in place) needs a dense array")
                dense = self.empty(a.shape, a.dtype)
                self.assign(dense, a)
                a = dense
            shape, strides, axis = (a.size,), (1,), 0
        else:
            (axis,) = self._axes(a.ndim, int(axis))
            shape, strides = tuple(a.shape), tuple(a.strides)
        if int(np.prod(shape, dtype=np.int64)) and shape[axis] - ddof <= 0:
            raise ValueError(f"{name}: N - ddof = {shape[axis]} - {ddof} is not positive")
        if out is None:
            out = self.empty(shape, a.dtype)
        elif out is a:
            if not a.is_dense():
                raise ValueError(f"{name}: out=a (in place) needs a dense array")
        elif out.dtype != a.dtype or tuple(out.shape) != tuple(shape) or not out.is_dense():
            raise ValueError(f"{name}: out must be a dense {a.dtype} array of shape {tuple(shape)}; "
                             f"got {out.dtype} {tuple(out.shape)} dense={out.is_dense()}")
        try:
            self._ck(self.c.smhip_standardize_axis(C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(axis),
                                                   C.c_double(eps), C.c_int64(ddof), C.c_void_p(out.ptr)))
        except SmhipError as e:
            if e.code == ERR_INVALID:
                raise ValueError(str(e)) from None
            raise
        return out

    def moments_raw(self, kind, dtype, a_ptr, shape, strides, mask, ddof=0, out_ptr=0, mean_ptr=0, ndim=None):
        """smhip_moments_axes with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        return self.c.smhip_moments_axes(C.c_int(kind), C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                         _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_uint32(mask), C.c_int64(ddof),
                                         C.c_void_p(out_ptr), C.c_void_p(mean_ptr))

    def standardize_raw(self, dtype, a_ptr, shape, strides, axis, eps=0.0, ddof=0, out_ptr=0, ndim=None):
        """smhip_standardize_axis with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        return self.c.smhip_standardize_axis(C.c_int(dtype), C.c_void_p(a_ptr), _i64(shape) if shape is not None else None,
                                             _i64(strides) if strides is not None else None, C.c_int(ndim), C.c_int(axis), C.c_double(eps),
                                             C.c_int64(ddof), C.c_void_p(out_ptr))

    def moments_plan(self, kind, dtype, shape, strides, axis, ddof=0):
        """smhip_moments_plan (host only): (route word, launches, (O, R, I), (L, reads, levels)) for a call on shape / strides (elements)."""
        kind = MOMENT_KINDS[kind] if isinstance(kind, str) else int(kind)
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        axes = self._axes(len(shape), axis)
        route, launches, ori, info = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), (C.c_int64 * 3)()
        self._ck(self.c.smhip_moments_plan(C.c_int(kind), C.c_int(dtype), _i64(shape), _i64(strides), C.c_int(len(shape)),
                                           C.c_uint32(sum(1 << d for d in axes)), C.c_int64(int(ddof)), C.byref(route), C.byref(launches), ori, info))
        return route.value, launches.value, tuple(int(x) for x in ori), tuple(int(x) for x in info)

    def standardize_plan(self, dtype, shape, strides, axis, eps=0.0, ddof=0):
        """smhip_standardize_plan (host only): the same four for standardize along `axis`."""
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        route, launches, ori, info = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), (C.c_int64 * 3)()
        self._ck(self.c.smhip_standardize_plan(C.c_int(dtype), _i64(shape), _i64(strides), C.c_int(len(shape)), C.c_int(int(axis)), C.c_double(float(eps)),
                                               C.c_int64(int(ddof)), C.byref(route), C.byref(launches), ori, info))
        return route.value, launches.value, tuple(int(x) for x in ori), tuple(int(x) for x in info)

    def take_along_axis(self, a: DeviceArray, idx: DeviceArray, axis, mode="checked", out: DeviceArray | None = None):
        """np.take_along_axis(a, idx, axis): out[..., j, ...] = a[..., idx[..., j, ...], ...] -> a new dense DeviceArray (or into
        `out`, a dense array of a's dtype and the result's element count, never an operand).  `idx` is an int64 DeviceArray of
        a's rank whose other axes equal a's or broadcast against them; both may be views.  axis=None flattens both row-major.
        mode: "checked" (numpy's rule: negatives count from the end, anything else out of range raises IndexError -- after
        reading the one-word flag, which waits for the stream), "clip" or "wrap" (np.take's, fully asynchronous)."""
        self._take_dtypes(a, idx)
        if axis is None:
            a, idx = self._flat(a), self._flat(idx)
            axis = 0
        if a.ndim != idx.ndim:
            raise ValueError(f"take_along_axis: a has rank {a.ndim}, idx rank {idx.ndim}")
        (axis,) = self._axes(a.ndim, int(axis))
        shape, sa, si = [], [], []
        for d in range(a.ndim):
            na, ni = a.shape[d], idx.shape[d]
            if d == axis:
                shape.append(ni), sa.append(a.strides[d]), si.append(idx.strides[d])
                continue
            if na != ni and na != 1 and ni != 1:
                raise ValueError(f"take_along_axis: shapes {a.shape} and {idx.shape} do not broadcast at axis {d}")
            n = ni if na == 1 else na
            shape.append(n), sa.append(a.strides[d] if na == n and n != 1 else 0), si.append(idx.strides[d] if ni == n and n != 1 else 0)
        return self._take(a, idx, sa, a.shape[axis], si, shape, axis, mode, out, tuple(shape), "take_along_axis")

    def take(self, a: DeviceArray, idx: DeviceArray, axis=None, mode="checked", out: DeviceArray | None = None):
        """np.take(a, idx, axis): a's shape with `axis` replaced by idx's shape (idx is an int64 DeviceArray, 1-D in the C ABI's
        terms; an N-D one is flattened and the result reshaped, as numpy does).  axis=None indexes a's row-major flattening.
        mode and out as in take_along_axis()."""
        self._take_dtypes(a, idx)
        if axis is None:
            a, axis = self._flat(a), 0
        (axis,) = self._axes(a.ndim, int(axis))
        if out is idx:
            raise ValueError("take: out must not be an operand")
        flat = idx if idx.ndim == 1 else self._flat(idx)
        shape = list(a.shape)
        shape[axis] = flat.size
        si = [0] * a.ndim
        si[axis] = flat.strides[0]
        result_shape = a.shape[:axis] + idx.shape + a.shape[axis + 1:]
        return self._take(a, flat, list(a.strides), a.shape[axis], si, shape, axis, mode, out, result_shape, "take")

    def _take_dtypes(self, a, idx):
        if a.dtype not in DTYPES:
            raise ValueError(f"take: dtype {a.dtype} (f32, f64, i32 and i64 only)")
        if idx.dtype != np.dtype(np.int64):
            raise ValueError(f"take: the index array must be int64, got {idx.dtype}")

    def _flat(self, a):
        """`a` in row-major order as a 1-D array: a view is copied dense first."""
        if not a.is_dense():
            dense = self.empty(a.shape, a.dtype)
            self.assign(dense, a)
            a = dense
        return DeviceArray(self, a.base_ptr, a.dtype, (a.size,), (1,), a.offset, a._owner)

    def _take(self, a, idx, sa, extent, si, shape, axis, mode, out, result_shape, who):
        if mode not in INDEX_MODES:
            raise ValueError(f"{who}: mode {mode!r} (one of 'checked', 'clip', 'wrap')")
        n = int(np.prod(shape, dtype=np.int64))
        if out is None:
            out = self.empty(result_shape, a.dtype)
        elif out is a or out is idx:
            raise ValueError(f"{who}: out must not be an operand")
        elif out.dtype != a.dtype or out.size != n or not out.is_dense():
            raise ValueError(f"{who}: out must be a dense {a.dtype} array of {n} elements (shape {tuple(result_shape)}); "
                             f"got {out.dtype} {out.shape} dense={out.is_dense()}")
        if n and extent == 0:
            raise IndexError(f"{who}: cannot take from an axis of 0 elements")
        checked = INDEX_MODES[mode] == INDEX_CHECKED and n > 0
        flag = self.empty((1,), np.int64) if checked else None
        self._ck(self.c.smhip_take_axis(C.c_int(INDEX_MODES[mode]), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), _i64(sa), C.c_int64(extent),
                                        C.c_void_p(idx.ptr), _i64(si), _i64(shape), C.c_int(len(shape)), C.c_int(axis), C.c_void_p(out.ptr),
                                        C.c_void_p(flag.ptr if checked else 0)))
        if checked and int(flag.numpy()[0]):
            raise IndexError(f"{who}: an index is out of bounds for axis {axis} with size {extent}")
        return out

    def take_raw(self, mode, dtype, a_ptr, a_strides, a_extent, idx_ptr, idx_strides, out_shape, axis, out_ptr, bad_ptr=0, ndim=None):
        """smhip_take_axis with every argument as given (argument-validation tests); ndim defaults to len(out_shape)."""
        if ndim is None:
            ndim = len(out_shape) if out_shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        return self.c.smhip_take_axis(C.c_int(mode), C.c_int(dtype), C.c_void_p(a_ptr), arr(a_strides), C.c_int64(a_extent), C.c_void_p(idx_ptr),
                                      arr(idx_strides), arr(out_shape), C.c_int(ndim), C.c_int(axis), C.c_void_p(out_ptr), C.c_void_p(bad_ptr))

    def take_plan(self, dtype, a_strides, a_extent, idx_strides, out_shape, axis, mode="clip"):
        """smhip_take_plan (host only): (route word, launches, (O, J, I), K) for a call with these strides (elements) over out_shape."""
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        mode = INDEX_MODES[mode] if not isinstance(mode, int) else mode
        route, launches, oji, chunk = C.c_int(0), C.c_int(0), (C.c_int64 * 3)(), C.c_int64(0)
        self._ck(self.c.smhip_take_plan(C.c_int(mode), C.c_int(dtype), _i64(a_strides), C.c_int64(int(a_extent)), _i64(idx_strides), _i64(out_shape),
                                        C.c_int(len(out_shape)), C.c_int(int(axis)), C.byref(route), C.byref(launches), oji, C.byref(chunk)))
        return route.value, launches.value, tuple(int(x) for x in oji), chunk.value

    def put_along_axis(self, a: DeviceArray, idx: DeviceArray, values, axis, mode="checked", unique=False):
        """np.put_along_axis(a, idx, values, axis), in place: a[..., pick(idx[..., j, ...]), ...] = values[..., j, ...]; returns `a`.
        `a` is a dense DeviceArray; `idx` an int64 DeviceArray of a's rank whose other axes equal a's or are 1; `values` a
        DeviceArray that broadcasts against idx (over a's other axes) or a Python scalar; both may be views.  Among entries of
        a line that name the same position the one with the largest j wins.  axis=None flattens a and idx row-major.
        mode: "checked" (negatives count from the end; an entry outside [-R, R) is dropped and IndexError raised after the
        launches -- the valid entries have been applied by then), "clip" or "wrap" (fully asynchronous).  unique=True is the
        caller's promise that no two entries of a line name the same position: one launch, no sort."""
        return self._scatter_along(SCATTER_PUT, a, idx, values, axis, mode, unique, "put_along_axis")

    def scatter_add(self, a: DeviceArray, idx: DeviceArray, values, axis, mode="checked", unique=False):
        """np.add.at along an axis (torch's scatter_add_), in place: a[..., pick(idx[..., j, ...]), ...] += values[..., j, ...],
        the contributions of a destination added one by one in ascending j (f32 in fp64, rounded once); returns `a`.
        Arguments as put_along_axis()."""
        return self._scatter_along(SCATTER_ADD, a, idx, values, axis, mode, unique, "scatter_add")

    def put(self, a: DeviceArray, ids: DeviceArray, values, axis=None, mode="checked", unique=False):
        """The inverse of take(a, ids, axis), in place: a[..., pick(ids[j]), ...] = values[..., j, ...]; returns `a`.  `ids` is a
        1-D int64 DeviceArray (an N-D one is flattened); `values` has a's shape with `axis` replaced by ids.size, or broadcasts
        to it, or is a Python scalar.  axis=None indexes a's row-major flattening (np.put).  mode and unique as in put_along_axis()."""
        return self._scatter_ids(SCATTER_PUT, a, ids, values, axis, mode, unique, "put")

    def index_add(self, a: DeviceArray, ids: DeviceArray, values, axis=None, mode="checked", unique=False):
        """torch's index_add_ / np.add.at(a, ids, values) along an axis, in place: a[..., pick(ids[j]), ...] += values[..., j, ...]
        in ascending j; returns `a`.  Arguments as put()."""
        return self._scatter_ids(SCATTER_ADD, a, ids, values, axis, mode, unique, "index_add")

    def _scatter_target(self, a, idx, values, who):
        if a.dtype not in DTYPES:
            raise ValueError(f"{who}: dtype {a.dtype} (f32, f64, i32 and i64 only)")
        if idx.dtype != np.dtype(np.int64):
            raise ValueError(f"{who}: the index array must be int64, got {idx.dtype}")
        if isinstance(values, DeviceArray) and values.dtype != a.dtype:
            raise ValueError(f"{who}: values are {values.dtype}, the target {a.dtype}")
        if a is idx or a is values:
            raise ValueError(f"{who}: the target must not be an operand")
        if not a.is_dense():
            raise ValueError(f"{who}: the target must be a dense array (scatter into a dense copy and assign it back)")

    def _scatter_along(self, kind, a, idx, values, axis, mode, unique, who):
        self._scatter_target(a, idx, values, who)
        if axis is None:
            a_flat, idx = self._flat(a), self._flat(idx)
            if isinstance(values, DeviceArray) and values.size != 1:
                values = self._flat(values)
            self._scatter_along(kind, a_flat, idx, values, 0, mode, unique, who)
            return a
        if a.ndim != idx.ndim:
            raise ValueError(f"{who}: the target has rank {a.ndim}, idx rank {idx.ndim}")
        (axis,) = self._axes(a.ndim, int(axis))
        si = []
        for d in range(a.ndim):
            na, ni = a.shape[d], idx.shape[d]
            if d != axis and ni != na and ni != 1:
                raise ValueError(f"{who}: shapes {a.shape} and {idx.shape} do not match at axis {d}")
            si.append(idx.strides[d] if d == axis or (ni == na and na != 1) else 0)
        self._scatter(kind, a, a.shape, axis, idx, si, values, idx.shape[axis], mode, unique, who)
        return a

    def _scatter_ids(self, kind, a, ids, values, axis, mode, unique, who):
        self._scatter_target(a, ids, values, who)
        flat = ids if ids.ndim == 1 else self._flat(ids)
        if axis is None:
            target, axis = self._flat(a), 0
        else:
            target = a
            (axis,) = self._axes(a.ndim, int(axis))
        si = [0] * target.ndim
        si[axis] = flat.strides[0]
        self._scatter(kind, target, target.shape, axis, flat, si, values, flat.size, mode, unique, who)
        return a

    def _scatter(self, kind, a, out_shape, axis, idx, si, values, J, mode, unique, who):
        if mode not in INDEX_MODES:
            raise ValueError(f"{who}: mode {mode!r} (one of 'checked', 'clip', 'wrap')")
        nd = len(out_shape)
        walk = [J if d == axis else out_shape[d] for d in range(nd)]
        if isinstance(values, DeviceArray):
            # numpy's rule, right-aligned: an extent of the values is the walk's or 1 (sm::broadcast, which smhip_broadcast follows, has no
            # empty extents: against (7, 0) it turns (7, 1) into (7, 1), and a call without entries would be refused here)
            pad = nd - values.ndim
            if pad < 0 or any(n != want and n != 1 for n, want in zip(values.shape, walk[pad:])):
                raise ValueError(f"{who}: values of shape {values.shape} do not broadcast to {tuple(walk)}")
            sv = [0] * pad + [st if n == want and n != 1 else 0 for n, st, want in zip(values.shape, values.strides, walk[pad:])]
        else:
            values = self.to_device(np.array([values], dtype=a.dtype))
            sv = [0] * nd
        n = int(np.prod(walk, dtype=np.int64))
        if n and out_shape[axis] == 0:
            raise IndexError(f"{who}: cannot place entries on an axis of 0 elements")
        checked = INDEX_MODES[mode] == INDEX_CHECKED and n > 0
        flag = self.empty((1,), np.int64) if checked else None
        self._ck(self.c.smhip_scatter_axis(C.c_int(kind), C.c_int(INDEX_MODES[mode]), C.c_int(SCATTER_UNIQUE if unique else 0), C.c_int(DTYPES[a.dtype]),
                                           C.c_void_p(a.ptr), _i64(out_shape), C.c_int(nd), C.c_int(axis), C.c_void_p(idx.ptr), _i64(si),
                                           C.c_void_p(values.ptr), _i64(sv), C.c_int64(J), C.c_void_p(flag.ptr if checked else 0)))
        if checked and int(flag.numpy()[0]):
            raise IndexError(f"{who}: an index is out of bounds for axis {axis} with size {out_shape[axis]} (the valid entries have been applied)")

    def scatter_raw(self, kind, mode, flags, dtype, out_ptr, out_shape, axis, idx_ptr, idx_strides, val_ptr, val_strides, n_entries, bad_ptr=0, ndim=None):
        """smhip_scatter_axis with every argument as given (argument-validation tests); ndim defaults to len(out_shape)."""
        if ndim is None:
            ndim = len(out_shape) if out_shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        return self.c.smhip_scatter_axis(C.c_int(kind), C.c_int(mode), C.c_int(flags), C.c_int(dtype), C.c_void_p(out_ptr), arr(out_shape), C.c_int(ndim),
                                         C.c_int(axis), C.c_void_p(idx_ptr), arr(idx_strides), C.c_void_p(val_ptr), arr(val_strides), C.c_int64(n_entries),
                                         C.c_void_p(bad_ptr))

    def scatter_plan(self, dtype, out_shape, axis, idx_strides, val_strides, n_entries, unique=False, kind=SCATTER_PUT, mode="clip"):
        """smhip_scatter_plan (host only): (route word, launches, (O, R, J, I), sorted entries) for a call with these strides
        (elements, against out_shape with `axis` replaced by n_entries)."""
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        mode = INDEX_MODES[mode] if not isinstance(mode, int) else mode
        route, launches, orji, nsorted = C.c_int(0), C.c_int(0), (C.c_int64 * 4)(), C.c_int64(0)
        self._ck(self.c.smhip_scatter_plan(C.c_int(kind), C.c_int(mode), C.c_int(SCATTER_UNIQUE if unique else 0), C.c_int(dtype), _i64(out_shape),
                                           C.c_int(len(out_shape)), C.c_int(int(axis)), _i64(idx_strides), _i64(val_strides), C.c_int64(int(n_entries)),
                                           C.byref(route), C.byref(launches), orji, C.byref(nsorted)))
        return route.value, launches.value, tuple(int(x) for x in orji), nsorted.value

    # -- counting -------------------------------------------------------------------
    def searchsorted(self, edges: DeviceArray, x: DeviceArray, side="left", out: DeviceArray | None = None):
        """np.searchsorted(edges, x, side) -> an int64 DeviceArray of x's shape (or into `out`, a dense int64 array of x's element
        count).  `edges` is a 1-D dense DeviceArray of x's dtype, sorted ascending as sort() sorts (NaNs last); `x` any view."""
        if side not in SIDES:
            raise ValueError(f"searchsorted: side {side!r} (one of 'left', 'right')")
        if x.dtype not in DTYPES or edges.dtype != x.dtype:
            raise ValueError(f"searchsorted: edges are {edges.dtype}, x {x.dtype} (the same one of f32, f64, i32, i64)")
        if edges.ndim != 1 or not edges.is_dense():
            raise ValueError("searchsorted: the edges must be a dense 1-D array")
        if out is None:
            out = self.empty(x.shape, np.int64)
        elif out is x or out is edges:
            raise ValueError("searchsorted: out must not be an operand")
        elif out.dtype != np.dtype(np.int64) or out.size != x.size or not out.is_dense():
            raise ValueError(f"searchsorted: out must be a dense int64 array of {x.size} elements; got {out.dtype} {out.shape} dense={out.is_dense()}")
        self._ck(self.c.smhip_searchsorted(C.c_int(SIDES[side]), C.c_int(DTYPES[x.dtype]), C.c_void_p(edges.ptr), C.c_int64(edges.size), C.c_void_p(x.ptr),
                                           _i64(x.shape), _i64(x.strides), C.c_int(x.ndim), C.c_void_p(out.ptr)))
        return out

    def bincount(self, ids: DeviceArray, nbins, mode="checked"):
        """counts[p] = how many of `ids` (an int32 or int64 DeviceArray, any view, read row-major) name position p of `nbins` -> an
        int64 DeviceArray of shape (nbins,).  The same bits as index_add(zeros, ids, 1, 0, mode).  mode: "checked" (negatives count
        from the end; an id outside [-nbins, nbins) is dropped and IndexError raised after the launches -- the valid ids have been
        counted by then), "clip" or "wrap" (fully asynchronous).  The length is never inferred from the data."""
        if mode not in INDEX_MODES:
            raise ValueError(f"bincount: mode {mode!r} (one of 'checked', 'clip', 'wrap')")
        if ids.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise ValueError(f"bincount: the ids must be int32 or int64, got {ids.dtype}")
        nbins = int(nbins)
        if nbins < 0 or (nbins == 0 and ids.size):
            raise ValueError(f"bincount: cannot count {ids.size} ids into {nbins} bins")
        counts = self.empty((nbins,), np.int64)
        checked = INDEX_MODES[mode] == INDEX_CHECKED and ids.size > 0
        flag = self.empty((1,), np.int64) if checked else None
        self._ck(self.c.smhip_bincount(C.c_int(INDEX_MODES[mode]), C.c_int(DTYPES[ids.dtype]), C.c_void_p(ids.ptr), _i64(ids.shape), _i64(ids.strides),
                                       C.c_int(ids.ndim), C.c_int64(nbins), C.c_void_p(counts.ptr), C.c_void_p(flag.ptr if checked else 0)))
        if checked and int(flag.numpy()[0]):
            raise IndexError(f"bincount: an id is out of bounds for {nbins} bins (the valid ids have been counted)")
        return counts

    def bincount_raw(self, mode, dtype, ids_ptr, shape, strides, nbins, counts_ptr, bad_ptr=0, ndim=None):
        """smhip_bincount with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        return self.c.smhip_bincount(C.c_int(mode), C.c_int(dtype), C.c_void_p(ids_ptr), arr(shape), arr(strides), C.c_int(ndim), C.c_int64(nbins),
                                     C.c_void_p(counts_ptr), C.c_void_p(bad_ptr))

    def searchsorted_raw(self, side, dtype, edges_ptr, n_edges, x_ptr, shape, strides, out_ptr, ndim=None):
        """smhip_searchsorted with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        return self.c.smhip_searchsorted(C.c_int(side), C.c_int(dtype), C.c_void_p(edges_ptr), C.c_int64(n_edges), C.c_void_p(x_ptr), arr(shape), arr(strides),
                                         C.c_int(ndim), C.c_void_p(out_ptr))

    def histogram_raw(self, flags, dtype, x_ptr, shape, strides, edges_ptr, bins, lo, hi, counts_ptr, ndim=None):
        """smhip_histogram with every argument as given (argument-validation tests); ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        return self.c.smhip_histogram(C.c_int(flags), C.c_int(dtype), C.c_void_p(x_ptr), arr(shape), arr(strides), C.c_int(ndim), C.c_void_p(edges_ptr),
                                      C.c_int64(bins), C.c_double(lo), C.c_double(hi), C.c_void_p(counts_ptr))

    def histogram_edges(self, bins, lo, hi, dtype):
        """smhip_histogram_edges (host only): np.linspace(lo, hi, bins + 1).astype(dtype) bit for bit, as a numpy array; ValueError
        where np.histogram(..., bins, range=(lo, hi)) raises."""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"histogram: a range needs float32 or float64 values, got {dtype}")
        bins = int(bins)
        edges = np.empty(max(bins, 0) + 1, dtype)
        rc = self.c.smhip_histogram_edges(C.c_int(DTYPES[dtype]), C.c_int64(bins), C.c_double(lo), C.c_double(hi), edges.ctypes.data_as(C.c_void_p))
        if rc == ERR_INVALID:
            raise ValueError(self.c.smhip_last_error().decode())
        self._ck(rc)
        return edges

    def histogram(self, x: DeviceArray, bins, range=None):
        """np.histogram.  histogram(x, bins, range=(lo, hi)) -> (counts, edges): `bins` equal bins over [lo, hi] for float32 / float64
        x; the edges are numpy's, as a DeviceArray of x's dtype.  histogram(x, edges) with `edges` a dense 1-D DeviceArray of x's
        dtype (f32, f64, i32, i64; non-decreasing, at least 2) -> counts.  counts is an int64 DeviceArray of shape (bins,); x is any
        view, read row-major.  The bin of a value is searchsorted(edges, v, "right") - 1, the last edge belongs to the last bin,
        values outside the edges and NaNs are not counted."""
        if x.dtype not in DTYPES:
            raise ValueError(f"histogram: dtype {x.dtype} (f32, f64, i32 and i64 only)")
        if isinstance(bins, DeviceArray):
            if range is not None:
                raise ValueError("histogram: explicit edges take no range")
            edges = bins
            if edges.dtype != x.dtype or edges.ndim != 1 or not edges.is_dense() or edges.size < 2:
                raise ValueError(f"histogram: the edges must be a dense 1-D {x.dtype} array of at least 2 elements")
            flags, nb, lo, hi, result = 0, edges.size - 1, 0.0, 0.0, None
        else:
            if range is None:
                raise ValueError("histogram: equal bins need range=(lo, hi) (the range is never inferred from the data)")
            lo, hi = float(range[0]), float(range[1])
            edges = self.to_device(self.histogram_edges(bins, lo, hi, x.dtype))
            flags, nb, result = HISTOGRAM_UNIFORM, int(bins), edges
        counts = self.empty((nb,), np.int64)
        self._ck(self.c.smhip_histogram(C.c_int(flags), C.c_int(DTYPES[x.dtype]), C.c_void_p(x.ptr), _i64(x.shape), _i64(x.strides), C.c_int(x.ndim),
                                        C.c_void_p(edges.ptr), C.c_int64(nb), C.c_double(lo), C.c_double(hi), C.c_void_p(counts.ptr)))
        return counts if result is None else (counts, result)

    def count_plan(self, what, dtype, shape, strides, bins, uniform=False, ndim=None):
        """smhip_count_plan (host only): (route word, launches, (workgroups, entries per slice, replicas, K, edges staged at most,
        staged)) for `what` ("searchsorted", "bincount", "histogram") over a view of these shape and strides (elements); `bins` is
        the number of edges for searchsorted, of bins otherwise."""
        what = COUNT_OPS[what] if not isinstance(what, int) else what
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        route, launches, info = C.c_int(0), C.c_int(0), (C.c_int64 * 6)()
        self._ck(self.c.smhip_count_plan(C.c_int(what), C.c_int(HISTOGRAM_UNIFORM if uniform else 0), C.c_int(dtype), arr(shape), arr(strides), C.c_int(ndim),
                                         C.c_int64(int(bins)), C.byref(route), C.byref(launches), info))
        return route.value, launches.value, tuple(int(v) for v in info)

    # -- choosing by condition --------------------------------------------------------
    def _cond(self, cond, who):
        """A condition -> (cmp, x, y or None, the scalar as a 1-element array of x's dtype or None).  `cond` is a DeviceArray
        (nonzero) or a tuple (x, "gt", rhs) with rhs a DeviceArray of x's dtype and shape or a Python / numpy scalar."""
        if isinstance(cond, DeviceArray):
            cond = (cond, "nonzero", None)
        if not (isinstance(cond, tuple) and len(cond) == 3 and isinstance(cond[0], DeviceArray)):
            raise ValueError(f"{who}: a condition is a DeviceArray or a tuple (x, cmp, rhs)")
        x, cmp, rhs = cond
        if x.dtype not in DTYPES:
            raise ValueError(f"{who}: dtype {x.dtype} (f32, f64, i32 and i64 only)")
        if cmp not in CMPS:
            raise ValueError(f"{who}: comparison {cmp!r} (one of {sorted(CMPS)})")
        if CMPS[cmp] == CMP_NONZERO:
            return CMP_NONZERO, x, None, None
        if isinstance(rhs, DeviceArray):
            if rhs.dtype != x.dtype:
                raise ValueError(f"{who}: the condition compares {x.dtype} with {rhs.dtype}")
            return CMPS[cmp], x, self._broadcast_to(rhs, x.shape, who), None
        if rhs is None:
            raise ValueError(f"{who}: comparison {cmp!r} needs a right-hand side")
        return CMPS[cmp], x, None, np.array([rhs]).astype(x.dtype)

    def _broadcast_to(self, d, shape, who):
        """`d` as a view over `shape` (numpy's rule: sizes of 1 and missing leading axes get stride 0)."""
        shape = tuple(shape)
        if d.shape == shape:
            return d
        if d.ndim > len(shape):
            raise ValueError(f"{who}: shape {d.shape} does not broadcast to {shape}")
        pad = len(shape) - d.ndim
        strides = [0] * pad
        for n, st, want in zip(d.shape, d.strides, shape[pad:]):
            if n != want and n != 1:
                raise ValueError(f"{who}: shape {d.shape} does not broadcast to {shape}")
            strides.append(st if n == want and n != 1 else 0)
        return DeviceArray(self, d.base_ptr, d.dtype, shape, strides, d.offset, d._owner)

    @staticmethod
    def _cond_args(cmp, x, y, s):
        return (C.c_int(cmp), C.c_int(DTYPES[x.dtype]), C.c_void_p(x.ptr), _i64(x.strides), C.c_void_p(y.ptr if y is not None else 0),
                _i64(y.strides) if y is not None else None, s.ctypes.data_as(C.c_void_p) if s is not None else None)

    def where(self, cond, a, b, out: DeviceArray | None = None):
        """np.where(cond, a, b) -> a dense DeviceArray of the condition's shape and dtype (or into `out`, which may be one of the
        operands when that one is dense: np.putmask).  `a` and `b` are each a DeviceArray of that dtype that broadcasts to the
        condition's shape, or a scalar.  The result holds the chosen operand's own bits.  Asynchronous."""
        cmp, x, y, s = self._cond(cond, "where")
        ops, keep = [], []
        for name, v in (("a", a), ("b", b)):
            if isinstance(v, DeviceArray):
                if v.dtype != x.dtype:
                    raise ValueError(f"where: {name} is {v.dtype}, the condition {x.dtype}")
                v = self._broadcast_to(v, x.shape, "where")
                ops += [C.c_void_p(v.ptr), _i64(v.strides), None]
            else:
                v = np.array([v]).astype(x.dtype)
                ops += [C.c_void_p(0), None, v.ctypes.data_as(C.c_void_p)]
            keep.append(v)   # alive until the call returns
        if out is None:
            out = self.empty(x.shape, x.dtype)
        elif out.dtype != x.dtype or out.shape != x.shape or not out.is_dense():
            raise ValueError(f"where: out must be a dense {x.dtype} array of shape {x.shape}")
        self._ck(self.c.smhip_where(*self._cond_args(cmp, x, y, s), *ops, _i64(x.shape), C.c_int(x.ndim), C.c_void_p(out.ptr)))
        del keep
        return out

    def count_nonzero(self, cond):
        """np.count_nonzero(cond) -> int.  THIS WAITS FOR THE STREAM: the count is read back from the device."""
        cmp, x, y, s = self._cond(cond, "count_nonzero")
        word = self.empty((1,), np.int64)
        self._ck(self.c.smhip_select_count(*self._cond_args(cmp, x, y, s), _i64(x.shape), C.c_int(x.ndim), C.c_void_p(word.ptr)))
        return self.read_i64(word.ptr)

    def _compact(self, what, cond, src, who):
        cmp, x, y, s = self._cond(cond, who)
        if src is not None:
            if src.shape != x.shape:
                raise ValueError(f"{who}: the array has shape {src.shape}, the condition {x.shape}")
            if src.dtype.itemsize not in (4, 8):
                raise ValueError(f"{who}: elements of {src.dtype.itemsize} bytes (4 or 8)")
        word = self.empty((1,), np.int64)
        args = self._cond_args(cmp, x, y, s)
        self._ck(self.c.smhip_select_count(*args, _i64(x.shape), C.c_int(x.ndim), C.c_void_p(word.ptr)))
        total = self.read_i64(word.ptr)   # waits for the stream
        planes = x.ndim if what == SELECT_COORDS else 1
        out = self.empty((planes * total,), src.dtype if src is not None else np.int64)
        self._ck(self.c.smhip_select(C.c_int(what), *args, _i64(x.shape), C.c_int(x.ndim), C.c_void_p(src.ptr if src is not None else 0),
                                     _i64(src.strides) if src is not None else None, C.c_int(src.dtype.itemsize if src is not None else 0),
                                     C.c_void_p(out.ptr), C.c_int64(total), None))
        return out, total

    def flatnonzero(self, cond):
        """np.flatnonzero(cond) -> an int64 DeviceArray of shape (count,): the row-major positions where the condition holds.
        THIS WAITS FOR THE STREAM ONCE, to learn the size: count, read it back, allocate exactly, select."""
        return self._compact(SELECT_INDEX, cond, None, "flatnonzero")[0]

    def nonzero(self, cond):
        """np.nonzero(cond) -> a tuple of ndim int64 DeviceArrays of shape (count,), one per axis.  THIS WAITS FOR THE STREAM ONCE,
        to learn the size."""
        out, total = self._compact(SELECT_COORDS, cond, None, "nonzero")
        ndim = cond.ndim if isinstance(cond, DeviceArray) else cond[0].ndim
        return tuple(DeviceArray(self, out.base_ptr, np.int64, (total,), (1,), d * total, out._owner) for d in range(ndim))

    def select(self, a: DeviceArray, cond):
        """a[mask] -> a DeviceArray of a's dtype and shape (count,): the elements of `a` where the condition holds, row-major.  `a`
        has the condition's shape and any 4- or 8-byte dtype.  THIS WAITS FOR THE STREAM ONCE, to learn the size."""
        return self._compact(SELECT_VALUES, cond, a, "select")[0]

    def where_raw(self, cmp, dtype, x_ptr, x_strides, y_ptr, y_strides, rhs, a_ptr, a_strides, a_scalar, b_ptr, b_strides, b_scalar, shape, out_ptr, ndim=None):
        """smhip_where with every argument as given (argument-validation tests); the scalars are numpy arrays of one element or
        None; ndim defaults to len(shape)."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        host = lambda v: v.ctypes.data_as(C.c_void_p) if v is not None else None  # noqa: E731
        return self.c.smhip_where(C.c_int(cmp), C.c_int(dtype), C.c_void_p(x_ptr), arr(x_strides), C.c_void_p(y_ptr), arr(y_strides), host(rhs),
                                  C.c_void_p(a_ptr), arr(a_strides), host(a_scalar), C.c_void_p(b_ptr), arr(b_strides), host(b_scalar), arr(shape),
                                  C.c_int(ndim), C.c_void_p(out_ptr))

    def select_count_raw(self, cmp, dtype, x_ptr, x_strides, y_ptr, y_strides, rhs, shape, count_ptr, ndim=None):
        """smhip_select_count with every argument as given; `rhs` a numpy array of one element or None."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        return self.c.smhip_select_count(C.c_int(cmp), C.c_int(dtype), C.c_void_p(x_ptr), arr(x_strides), C.c_void_p(y_ptr), arr(y_strides),
                                         rhs.ctypes.data_as(C.c_void_p) if rhs is not None else None, arr(shape), C.c_int(ndim), C.c_void_p(count_ptr))

    def select_raw(self, what, cmp, dtype, x_ptr, x_strides, y_ptr, y_strides, rhs, shape, src_ptr, src_strides, src_elem_bytes, out_ptr, capacity, count_ptr=0,
                   ndim=None):
        """smhip_select with every argument as given; `rhs` a numpy array of one element or None."""
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        return self.c.smhip_select(C.c_int(what), C.c_int(cmp), C.c_int(dtype), C.c_void_p(x_ptr), arr(x_strides), C.c_void_p(y_ptr), arr(y_strides),
                                   rhs.ctypes.data_as(C.c_void_p) if rhs is not None else None, arr(shape), C.c_int(ndim), C.c_void_p(src_ptr), arr(src_strides),
                                   C.c_int(src_elem_bytes), C.c_void_p(out_ptr), C.c_int64(capacity), C.c_void_p(count_ptr))

    def select_plan(self, what, dtype, shape, x_strides, y_strides=None, a_strides=None, b_strides=None, cmp=CMP_GT, ndim=None):
        """smhip_select_plan (host only): (route word, launches, (tiles, elements per tile, the largest element count of the
        one-workgroup route, operands copied)) for `what` ("index", "coords", "values", "count", "where") over a condition of this
        shape; strides in elements, None for a scalar or an operand the call does not have."""
        what = SELECT_OPS[what] if not isinstance(what, int) else what
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        if ndim is None:
            ndim = len(shape) if shape is not None else 0
        arr = lambda v: _i64(v) if v is not None else None  # noqa: E731
        route, launches, info = C.c_int(0), C.c_int(0), (C.c_int64 * 4)()
        self._ck(self.c.smhip_select_plan(C.c_int(what), C.c_int(cmp), C.c_int(dtype), arr(shape), C.c_int(ndim), arr(x_strides), arr(y_strides), arr(a_strides),
                                          arr(b_strides), C.byref(route), C.byref(launches), info))
        return route.value, launches.value, tuple(int(v) for v in info)

    # -- the distinct values --------------------------------------------------------
    def unique(self, a: DeviceArray, return_index=False, return_inverse=False, return_counts=False, equal_nan=True):
        """np.unique(a, return_index, return_inverse, return_counts, equal_nan=equal_nan) of the row-major flattening of `a` (any view):
        the distinct values ascending, one NaN last (every NaN with equal_nan=False), as a DeviceArray of shape (U,) holding the bits of
        each value's FIRST occurrence -- alone, or a tuple with, in numpy's order, the int64 arrays asked for: `index` (U,) the first
        occurrence, `inverse` of a's shape (values.take(inverse) rebuilds a), `counts` (U,).  One stable sort, the count of the runs,
        then one emitting call.  THIS WAITS FOR THE STREAM ONCE, to learn U.  a.size >= 2^31 raises what sort() raises."""
        if a.dtype not in DTYPES:
            raise ValueError(f"unique: dtype {a.dtype} (f32, f64, i32 and i64 only)")
        flat = self._flat(a)
        order = None
        if flat.size:
            got = self._sort(flat, 0, False, True, return_index or return_inverse, None, None)
            flat, order = got if isinstance(got, tuple) else (got, None)
        return self._runs(flat, order, a.shape, return_index, return_inverse, return_counts, equal_nan)

    def unique_consecutive(self, a: DeviceArray, return_inverse=False, return_counts=False, equal_nan=True):
        """torch.unique_consecutive / run-length encoding of the row-major flattening of `a`: the first element of every run of adjacent
        elements that are the same (-0.0 == +0.0; NaNs the same among themselves unless equal_nan=False), shape (U,) -- alone, or a tuple
        with `inverse` (a's shape: the run each element lies in) and / or `counts` (U,: the runs' lengths).  No sort, no size limit.
        THIS WAITS FOR THE STREAM ONCE, to learn U."""
        if a.dtype not in DTYPES:
            raise ValueError(f"unique_consecutive: dtype {a.dtype} (f32, f64, i32 and i64 only)")
        return self._runs(self._flat(a), None, a.shape, False, return_inverse, return_counts, equal_nan)

    def _runs(self, flat, order, shape, want_index, want_inverse, want_counts, equal_nan):
        """Count the runs of `flat` (dense, 1-D), read the count back, allocate exactly, emit."""
        flags, dt, n = C.c_int(0 if equal_nan else RUNS_NAN_DISTINCT), C.c_int(DTYPES[flat.dtype]), flat.size
        total = 0
        if n:
            word = self.empty((1,), np.int64)
            self._ck(self.c.smhip_runs_count(flags, dt, C.c_void_p(flat.ptr), C.c_int64(n), C.c_void_p(word.ptr)))
            total = self.read_i64(word.ptr)   # waits for the stream
        values = self.empty((total,), flat.dtype)
        index = self.empty((total,), np.int64) if want_index else None
        inverse = self.empty(shape, np.int64) if want_inverse else None
        counts = self.empty((total,), np.int64) if want_counts else None
        if n:
            ptr = lambda d: C.c_void_p(d.ptr if d is not None else 0)  # noqa: E731
            self._ck(self.c.smhip_runs(flags, dt, C.c_void_p(flat.ptr), C.c_int64(n), ptr(order), ptr(values), ptr(index), ptr(counts), ptr(inverse),
                                       C.c_int64(total), None))
        out = (values,) + tuple(r for r in (index, inverse, counts) if r is not None)
        return out[0] if len(out) == 1 else out

    def runs_count_raw(self, flags, dtype, s_ptr, n, count_ptr):
        """smhip_runs_count with every argument as given (argument-validation tests)."""
        return self.c.smhip_runs_count(C.c_int(flags), C.c_int(dtype), C.c_void_p(s_ptr), C.c_int64(n), C.c_void_p(count_ptr))

    def runs_raw(self, flags, dtype, s_ptr, n, order_ptr, values_ptr, index_ptr, counts_ptr, inverse_ptr, capacity, count_ptr=0):
        """smhip_runs with every argument as given; a pointer of 0 is NULL."""
        return self.c.smhip_runs(C.c_int(flags), C.c_int(dtype), C.c_void_p(s_ptr), C.c_int64(n), C.c_void_p(order_ptr), C.c_void_p(values_ptr),
                                 C.c_void_p(index_ptr), C.c_void_p(counts_ptr), C.c_void_p(inverse_ptr), C.c_int64(capacity), C.c_void_p(count_ptr))

    def runs_plan(self, dtype, n, outputs=RUNS_VALUES, flags=0):
        """smhip_runs_plan (host only): (route, launches, (tiles, elements per tile, the largest n of the one-workgroup route)) for the
        results in `outputs` (RUNS_* ORed; 0: the count alone) over n elements."""
        dtype = DTYPES[np.dtype(dtype)] if not isinstance(dtype, int) else dtype
        route, launches, info = C.c_int(0), C.c_int(0), (C.c_int64 * 3)()
        self._ck(self.c.smhip_runs_plan(C.c_int(flags), C.c_int(dtype), C.c_int64(n), C.c_int(outputs), C.byref(route), C.byref(launches), info))
        return route.value, launches.value, tuple(int(v) for v in info)

    def sum(self, a: DeviceArray):
        out = C.c_double(0)
        self._ck(self.c.smhip_sum(C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), C.c_size_t(a.size), C.byref(out)))
        return out.value

    def sum_async(self, a: DeviceArray, out_ptr):
        self._ck(self.c.smhip_sum_async(C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), C.c_size_t(a.size), C.c_void_p(out_ptr)))

    def dot_async(self, a: DeviceArray, b: DeviceArray, out_ptr):
        self._ck(self.c.smhip_dot_async(C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), C.c_void_p(b.ptr), C.c_size_t(a.size),
                                        C.c_void_p(out_ptr)))

    def dot_c64_async(self, a_ptr, b_ptr, n, out2_ptr):
        self._ck(self.c.smhip_dot_c64_async(C.c_void_p(a_ptr), C.c_void_p(b_ptr), C.c_size_t(n), C.c_void_p(out2_ptr)))

    def contiguous_sum_async(self, op, a: DeviceArray, b: DeviceArray, out: DeviceArray, sum_ptr):
        self._ck(self.c.smhip_contiguous_sum_async(C.c_int(op), C.c_int(DTYPES[a.dtype]), C.c_void_p(a.ptr), C.c_void_p(b.ptr),
                                                   C.c_void_p(out.ptr), C.c_size_t(a.size), C.c_void_p(sum_ptr)))

    def read_f64(self, ptr):
        out = np.zeros(1, dtype=np.float64)
        self.download(out, ptr)
        return float(out[0])

    def read_i64(self, ptr):
        out = np.zeros(1, dtype=np.int64)
        self.download(out, ptr)
        return int(out[0])

    # -- multi-GPU ----------------------------------------------------------------
    def split_range(self, n, world, rank):
        st, ct = C.c_int64(0), C.c_int64(0)
        self._ck(self.c.smhip_split_range(C.c_int64(n), C.c_int(world), C.c_int(rank), C.byref(st), C.byref(ct)))
        return st.value, ct.value

    def shard_outer(self, shape, strides_a, strides_b, world, rank):
        """The C planner behind sm::Sharded / smhip_sharded_elementwise; same answer as simplemath_amd.sharding.shard_outer."""
        nd = len(shape)
        local = _i64([0] * nd)
        oa, ob, oo = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        mask = C.c_int(0)
        self._ck(self.c.smhip_shard_outer(_i64(shape), _i64(strides_a), _i64(strides_b), C.c_int(nd), C.c_int(world), C.c_int(rank),
                                          local, C.byref(oa), C.byref(ob), C.byref(oo), C.byref(mask)))
        return tuple(local[:nd]), oa.value, ob.value, oo.value, bool(mask.value & 1), bool(mask.value & 2)

    def set_devices(self, n):
        self._ck(self.c.smhip_set_devices(C.c_int(n)))

    def get_devices(self):
        n = C.c_int(0)
        self._ck(self.c.smhip_get_devices(C.byref(n)))
        return n.value

    def group_info(self, index):
        """(nranks, rank, device) as RCCL reports them for the device group's communicator `index`."""
        n, r, d = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.c.smhip_group_info(C.c_int(index), C.byref(n), C.byref(r), C.byref(d)))
        return n.value, r.value, d.value

    def rccl_version(self):
        v = C.c_int(0)
        self._ck(self.c.smhip_rccl_version(C.byref(v)))
        return v.value

    def copy_peer(self, dst_ptr, dst_device, src_ptr, src_device, nbytes):
        self._ck(self.c.smhip_copy_peer(C.c_void_p(dst_ptr), C.c_int(dst_device), C.c_void_p(src_ptr), C.c_int(src_device), C.c_size_t(nbytes)))

    def sharded_synchronize(self):
        self._ck(self.c.smhip_sharded_synchronize())

    @staticmethod
    def _ptr_table(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    @staticmethod
    def _size_table(ns):
        return (C.c_size_t * len(ns))(*ns)

    def sharded_contiguous(self, op, dtype, a_ptrs, b_ptrs, out_ptrs, ns):
        self._ck(self.c.smhip_sharded_contiguous(C.c_int(op), C.c_int(DTYPES[np.dtype(dtype)]), self._ptr_table(a_ptrs),
                                                 self._ptr_table(b_ptrs), self._ptr_table(out_ptrs), self._size_table(ns)))

    def sharded_array_scalar(self, op, dtype, a_ptrs, value, ns, out_ptrs):
        v = np.array([value], dtype=dtype)
        self._ck(self.c.smhip_sharded_array_scalar(C.c_int(op), C.c_int(DTYPES[np.dtype(dtype)]), self._ptr_table(a_ptrs),
                                                   v.ctypes.data_as(C.c_void_p), self._size_table(ns), self._ptr_table(out_ptrs)))

    def sharded_elementwise(self, op, dtype, a_ptrs, sa, b_ptrs, sb, shape, out_ptrs):
        self._ck(self.c.smhip_sharded_elementwise(C.c_int(op), C.c_int(DTYPES[np.dtype(dtype)]), self._ptr_table(a_ptrs), _i64(sa),
                                                  self._ptr_table(b_ptrs), _i64(sb), _i64(shape), C.c_int(len(shape)),
                                                  self._ptr_table(out_ptrs)))

    def sharded_contiguous_sum(self, op, dtype, a_ptrs, b_ptrs, out_ptrs, ns):
        total = C.c_double(0)
        self._ck(self.c.smhip_sharded_contiguous_sum(C.c_int(op), C.c_int(DTYPES[np.dtype(dtype)]), self._ptr_table(a_ptrs),
                                                     self._ptr_table(b_ptrs), self._ptr_table(out_ptrs), self._size_table(ns),
                                                     C.byref(total)))
        return total.value

    def sharded_sum(self, dtype, a_ptrs, ns):
        total = C.c_double(0)
        self._ck(self.c.smhip_sharded_sum(C.c_int(DTYPES[np.dtype(dtype)]), self._ptr_table(a_ptrs), self._size_table(ns), C.byref(total)))
        return total.value

    def sharded_dot(self, dtype, a_ptrs, b_ptrs, ns):
        out = np.zeros(1, dtype=dtype)
        self._ck(self.c.smhip_sharded_dot(C.c_int(DTYPES[np.dtype(dtype)]), self._ptr_table(a_ptrs), self._ptr_table(b_ptrs),
                                          self._size_table(ns), out.ctypes.data_as(C.c_void_p)))
        return out[0]

    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._ck(self.c.smhip_comm_unique_id(buf))
        return buf.raw

    def comm_init_rank(self, nranks, rank, unique_id: bytes):
        assert len(unique_id) == 128
        self._ck(self.c.smhip_comm_init_rank(C.c_int(nranks), C.c_int(rank), C.c_char_p(unique_id)))

    def comm_info(self):
        n, r = C.c_int(0), C.c_int(0)
        self._ck(self.c.smhip_comm_info(C.byref(n), C.byref(r)))
        return n.value, r.value

    def comm_destroy(self):
        self._ck(self.c.smhip_comm_destroy())

    def allreduce_sum_async(self, dtype, ptr, count=1):
        self._ck(self.c.smhip_allreduce_sum_async(C.c_int(DTYPES[np.dtype(dtype)]), C.c_void_p(ptr), C.c_size_t(count)))

    def policy_probe(self, a=0, a_bytes=0, b=0, b_bytes=0, out=0, out_bytes=0):
        """The stream-policy word for a launch with these operand spans (bit 0: nt reads, bit 1: keep-stores); records the touches."""
        pol = C.c_int(0)
        self._ck(self.c.smhip_policy_probe(C.c_void_p(a), C.c_size_t(a_bytes), C.c_void_p(b), C.c_size_t(b_bytes), C.c_void_p(out),
                                           C.c_size_t(out_bytes), C.byref(pol)))
        return pol.value

    def policy_peek(self, a=0, a_bytes=0, b=0, b_bytes=0, out=0, out_bytes=0):
        """policy_probe without recording the spans as touched."""
        pol = C.c_int(0)
        self._ck(self.c.smhip_policy_peek(C.c_void_p(a), C.c_size_t(a_bytes), C.c_void_p(b), C.c_size_t(b_bytes), C.c_void_p(out),
                                          C.c_size_t(out_bytes), C.byref(pol)))
        return pol.value

    def queue_stats(self):
        """(queues in use on this thread's device, operators that took the other queue, cross-queue event edges)"""
        q, alt, edges = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._ck(self.c.smhip_queue_stats(C.byref(q), C.byref(alt), C.byref(edges)))
        return q.value, alt.value, edges.value

    def tiny_stats(self):
        """(launches that carried recorded tiny operators, operators they carried) on this thread's device (csrc/tiny.hip)"""
        launches, ops = C.c_ulonglong(0), C.c_ulonglong(0)
        self._ck(self.c.smhip_tiny_stats(C.byref(launches), C.byref(ops)))
        return launches.value, ops.value

    def launch_pieces(self, bytes_per_operand, streams=3):
        """Kernel launches a dense streaming operator over operands of this size goes out as (streams: 3 a op b, 2 a op s / dot, 1 sum)."""
        k = C.c_int(0)
        self._ck(self.c.smhip_launch_pieces(C.c_size_t(bytes_per_operand), C.c_int(streams), C.byref(k)))
        return k.value

    # -- timing -----------------------------------------------------------------
    def event(self):
        e = C.c_void_p(0)
        self._ck(self.c.smhip_event_create(C.byref(e)))
        return e.value

    def record(self, ev):
        self._ck(self.c.smhip_event_record(C.c_void_p(ev)))

    def event_sync(self, ev):
        self._ck(self.c.smhip_event_synchronize(C.c_void_p(ev)))

    def elapsed_ms(self, e0, e1):
        ms = C.c_float(0)
        self._ck(self.c.smhip_event_elapsed_ms(C.c_void_p(e0), C.c_void_p(e1), C.byref(ms)))
        return ms.value

    def event_destroy(self, ev):
        self._ck(self.c.smhip_event_destroy(C.c_void_p(ev)))


_lib = None


class Generator:
    """lib.generator(seed, stream=0): draws born on the device, element i a pure function of (seed, stream, offset, i) (smhip_random;
    smhip.h has the table, tests/random_model.py the CPU model).  Every method returns a new dense DeviceArray of `shape`, or fills
    `out` (a dense DeviceArray of the draw's dtype; `shape` is then ignored) in place; each advances `offset` by the blocks consumed.
    A kind that is not defined for the element type raises TypeError, parameters the C ABI refuses raise ValueError."""

    def __init__(self, lib, seed, stream=0):
        self.lib, self.seed, self.stream, self.offset = lib, int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1), 0

    def seek(self, blocks):
        self.offset = int(blocks)

    def _draw(self, who, kind, shape, dtype, params, out):
        lib = self.lib
        if out is not None:
            if dtype is not None and np.dtype(dtype) != out.dtype:
                raise TypeError(f"{who}: out is {out.dtype}, the draw is {np.dtype(dtype)}")
            dtype = out.dtype
        kind, dt = lib._random_pair(kind, dtype, who)
        if out is None:
            out = lib.empty(shape, dt)
        elif not out.is_dense():
            raise ValueError(f"{who}: out must be dense")
        n = out.size
        blocks = lib.random_blocks(kind, dt, n)
        rc = lib.random_raw(kind, DTYPES[dt], out.ptr if n else 0, n, self.seed, self.stream, self.offset, params)
        if rc == ERR_INVALID:
            raise ValueError(lib.c.smhip_last_error().decode())
        lib._ck(rc)
        self.offset += blocks
        return out

    def uniform(self, shape=None, lo=0.0, hi=1.0, dtype=None, out=None):
        """[lo, hi): float32 (the default) or float64."""
        return self._draw("uniform", RANDOM_UNIFORM, shape, dtype if dtype is not None or out is not None else np.float32, (float(lo), float(hi)), out)

    def normal(self, shape=None, mean=0.0, std=1.0, dtype=None, out=None):
        return self._draw("normal", RANDOM_NORMAL, shape, dtype if dtype is not None or out is not None else np.float32, (float(mean), float(std)), out)

    def integers(self, lo, hi, shape=None, dtype=None, out=None):
        """[lo, hi), 1 <= hi - lo <= 2^32: int64 (the default) or int32."""
        lo, hi = int(lo), int(hi)
        if int(float(lo)) != lo or int(float(hi)) != hi:
            raise ValueError(f"integers: the bounds {lo}, {hi} are not whole numbers of a double")
        return self._draw("integers", RANDOM_INTEGERS, shape, dtype if dtype is not None or out is not None else np.int64, (float(lo), float(hi)), out)

    def bernoulli(self, p, shape=None, dtype=None, out=None):
        """1 with probability p, else 0, in any of the four element types (float32 by default)."""
        return self._draw("bernoulli", RANDOM_BERNOULLI, shape, dtype if dtype is not None or out is not None else np.float32, (float(p), 0.0), out)

    def bits(self, shape=None, dtype=None, out=None):
        return self._draw("bits", RANDOM_BITS, shape, dtype if dtype is not None or out is not None else np.int64, None, out)

    def permutation(self, n, out=None):
        """A random order of 0 .. n - 1 (int64): the stable argsort of n 64-bit keys."""
        return self.lib.argsort(self.bits((int(n),), np.int64), axis=None, out=out)

    def shuffle(self, a, axis=0, out=None):
        """take(a, permutation(a.shape[axis]), axis)."""
        axis = axis + a.ndim if axis < 0 else axis
        if not 0 <= axis < a.ndim:
            raise ValueError(f"shuffle: axis {axis} of an array of rank {a.ndim}")
        return self.lib.take(a, self.permutation(a.shape[axis]), axis, mode="clip", out=out)


def load(path: str = LIB_PATH) -> Smhip:
    """The loaded library (cached).  Raises if libsmhip.so has not been built.  SMHIP_LIBRARY=<path> substitutes an
    experimental build (tools/build_variant.sh) for the default one."""
    global _lib
    if path == LIB_PATH and os.environ.get("SMHIP_LIBRARY"):
        path = os.environ["SMHIP_LIBRARY"]
    if _lib is None or _lib.path != path:
        _lib = Smhip(path)
    return _lib
