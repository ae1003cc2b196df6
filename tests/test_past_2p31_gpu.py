"""sort, take and scatter on operands of more than 2^31 elements and 4 GiB: the shapes of tests/large_cases.py (whose plans
test_past_2p31_host.py pins on the CPU) run on the device, against numpy alone, bit for bit.

What these sizes reach and the small shapes of test_sort_gpu.py / test_take_gpu.py / test_scatter_gpu.py cannot: `line * stride +
position` and `row * R + offset` past 2^31 elements and 2^32 / 2^33 / 2^34 bytes, div_small's arguments crossing 2^32 inside one
launch, grids at the cap of 2^20 workgroups whose task loops run more than once, the staged copies of a sort along a leading
axis, and positions R that do not fit 32 bits.

Operands are made on the device (smhip.uniform_f32) and any window of them is regenerated on the host (oracle.uniform_f32, the
same counter-based generator); an eight-byte operand is the same buffer behind an int64 DeviceArray.  Nothing large is uploaded or
downloaded: index arrays are small, one index array shared by every line is a stride-0 view, and results are read at the lines
large_cases.boundary_lines names (the first, those around element 2^31 and bytes 2^32 / 2^33, 16 past element 2^31, the last).
The reference is np.sort / np.argsort(kind="stable") (test_sort_gpu.reference), fancy indexing, and test_scatter_gpu.reference on a
compact table of the rows the entries name; every comparison is of bytes (scatter-add: test_scatter_gpu.same).  The one
tolerance is the whole-target sum of the scatter tests, see stray_sum().

Each test states its peak device memory (library scratch included).  The `device_memory` fixture frees whatever a test still
holds -- after a failed assertion too, when the traceback keeps the test's arrays alive -- and trims the pool, so the peak of the
file is the peak of one test: 40 GiB (S2).  No test trims the pool itself, so what the pool holds when a test ends is the most
it ever held; the fixture prints it."""
import ctypes as C
import math
import weakref

import numpy as np
import pytest

import simplemath_amd as sma
from tests import large_cases as lc
from tests.large_cases import P31, P32, boundary_lines
from tests.test_scatter_gpu import GARBAGE
from tests.test_scatter_gpu import normalise as scatter_normalise
from tests.test_scatter_gpu import reference as scatter_reference
from tests.test_scatter_gpu import same
from tests.test_sort_gpu import reference as sort_reference
from tests.test_sort_gpu import specials
from tests.test_take_gpu import normalise as take_normalise

pytestmark = pytest.mark.gpu

MODES = ("checked", "clip", "wrap")
PUT, ADD = sma.SCATTER_PUT, sma.SCATTER_ADD
KINDS = dict(argvalues=(PUT, ADD), ids=("put", "add"))
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
f32 = np.float32
ROWS, COLS = lc.TABLE_ROWS, lc.TABLE_COLS
# the rows of the (2^21 + 5, 1024) table around element 2^31 and byte 2^32, and the same rows counted from the end
BOUNDARY_ROWS = [0, (1 << 20) - 1, 1 << 20, (1 << 21) - 1, 1 << 21, (1 << 21) + 4, -1, -5, -ROWS]
# ... six distinct rows through both forms, for the calls that promise distinct positions
DISTINCT_ROWS = [(1 << 20) - 1, 1 << 20, (1 << 21) - 1, -5, -1, -ROWS]
FLAT_VALID = [0, P31 - 1, P31, lc.FLAT - 1, -1, -lc.FLAT, -P31]
FLAT_BAD = [lc.FLAT, -lc.FLAT - 1, P32, lc.FLAT + P32]


# ------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(autouse=True)
def device_memory(smhip, monkeypatch, request):
    """Every device block a test allocates through the binding is handed back when the test ends, passed or failed, and the pool
    is trimmed: a red test must not leave 8 - 32 GiB behind for the next one to trip over."""
    owners = []
    init = sma._Owner.__init__

    def recording(self, lib, ptr):
        init(self, lib, ptr)
        owners.append(weakref.ref(self))

    monkeypatch.setattr(sma._Owner, "__init__", recording)
    yield
    for ref in owners:
        owner = ref()
        if owner is not None and owner.ptr:
            smhip.free(owner.ptr)
            owner.ptr = 0   # its __del__ then frees nothing
    in_use, cached = smhip.pool_stats()
    print(f"device memory of {request.node.name}: the pool held {(in_use + cached) / 2 ** 30:.2f} GiB at most, {in_use / 2 ** 30:.2f} GiB still in use")
    smhip.pool_trim()


def view(lib, d, dtype, shape, strides=None, offset=0):
    """The buffer of `d` behind another dtype / shape / strides (elements of `dtype`)."""
    shape = [int(n) for n in shape]
    if strides is None:
        strides = [int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape))]
    return sma.DeviceArray(lib, d.base_ptr, dtype, shape, strides, offset, d._owner)


def window(lib, d, first, count, dtype=f32):
    """`count` elements of `dtype` from element `first` of d's buffer."""
    h = np.empty(count, dtype)
    lib.download(h, d.base_ptr + first * h.itemsize)
    return h


def generated(oracle, seed, first, count):
    """What uniform_f32(n, seed, 0, 1) holds at [first, first + count)."""
    return oracle.uniform_f32(count, seed, 0.0, 1.0, first=first)


def refill(lib, d, n, seed):
    lib._ck(lib.c.smhip_fill_uniform_f32(C.c_void_p(d.base_ptr), n, seed, 0, 0.0, 1.0))


def planned(lib, name):
    """The case, after checking that it still plans as the host test pinned it."""
    case = lc.CASES[name]
    assert lc.plan_of(lib, case) == (case["plan"], case["launches"]), name
    return case


def i64(*parts):
    """The parts (lists or arrays of integers) as one int64 array, nothing passing through a float."""
    return np.concatenate([np.asarray(part, np.int64).reshape(-1) for part in parts])


def flag_word(lib):
    return lib.to_device(np.array([GARBAGE], np.int64))


def rows_table(oracle, seed, rows, R):
    """-> (the distinct rows ascending, their R generated elements each)."""
    uniq = np.unique(np.asarray(rows, np.int64))
    return uniq, np.stack([generated(oracle, seed, int(r) * R, R) for r in uniq])


# ------------------------------------------------------------------------------------------------------ sort
def sort_rows(lib, oracle, name, seed, mode):
    """A case sorted along its last axis; mode: "both" (values and positions), "inplace" (values over the operand)."""
    case = planned(lib, name)
    dtype = case["dtype"]
    L, R = case["shape"]
    words = dtype.itemsize // 4
    lines = boundary_lines(L, R, (dtype.itemsize, 8) if mode == "both" else (dtype.itemsize,))
    plain = [x + 3 for x in lines if x + 3 < L and x + 3 not in lines]       # lines that keep the generator's values
    special = specials((len(lines), R), dtype.type, seed)                  # NaNs, both zeros, infinities, ties: over the sampled lines
    inputs = [(line, special[k]) for k, line in enumerate(lines)]
    inputs += [(line, generated(oracle, seed, line * R * words, R * words).view(dtype)) for line in plain]
    for descending in (False, True):
        buf = lib.uniform_f32(L * R * words, seed, 0.0, 1.0)
        a = view(lib, buf, dtype, (L, R))
        assert list(a.strides) == case["strides"]
        for k, line in enumerate(lines):
            lib.upload(buf.base_ptr + line * R * dtype.itemsize, special[k])
        idx = None
        if mode == "both":
            vals, idx = lib.sort(a, 1, descending, indices=True)
        else:
            vals = lib.sort(a, 1, descending, out=a)
            assert vals is a
        for line, x in inputs:
            want_v, want_i = sort_reference(x.reshape(1, R), 1, descending)
            assert window(lib, vals, line * R, R, dtype).tobytes() == want_v.tobytes(), (name, descending, line, "values")
            if idx is not None:
                assert np.array_equal(window(lib, idx, line * R, R, np.int64), want_i[0]), (name, descending, line, "positions")
        del a, vals, idx, buf   # back to the pool: the descending pass takes the same blocks again


def test_sort_rows_of_1000(smhip, oracle):
    """S1: f32 (2 147 500, 1000) along the last axis, values and positions: ROW.  16 lines lie past element 2^31; the values pass
    byte 2^33 and the int64 positions bytes 2^32, 2^33 and 2^34.  Peak 32 GiB: operand 8, values 8, positions 16."""
    sort_rows(smhip, oracle, "S1", 41, "both")


def test_sort_rows_of_1000_as_int64(smhip, oracle):
    """S1's buffer as int64 (2 147 500, 500): a ROW sort of eight-byte elements whose outputs pass byte 2^33.  Peak 24 GiB:
    operand 8, values 8, positions 8."""
    sort_rows(smhip, oracle, "S1_i64", 42, "both")


def test_sort_rows_of_8193_in_place(smhip, oracle):
    """S2: f32 (262 129, 8193) in place: three tiles a line and two merge passes over pairs past element 2^31.  Peak 40 GiB:
    operand 8, the two pair buffers 2 x 16."""
    sort_rows(smhip, oracle, "S2", 43, "inplace")


def column_runs(cols, positions, width=8):
    """Disjoint runs (first column, columns) that cover `width` columns at each position."""
    cover = sorted({c for p in positions for c in range(min(p, cols - width), min(p, cols - width) + width)})
    runs, start = [], 0
    for k in range(1, len(cover) + 1):
        if k == len(cover) or cover[k] != cover[k - 1] + 1:
            runs.append((cover[start], k - start))
            start = k
    return runs


def sort_columns(lib, oracle, name, seed):
    """A case sorted along axis 0 of (rows, cols): the lines are columns, staged through a transposed copy in and out.  Columns are
    written and read as `rows` short transfers each, so nothing but the sort touches the large arrays."""
    case = planned(lib, name)
    rows, cols = case["shape"]
    positions = boundary_lines(cols, rows, (4,))                      # the lines of the staged rows [cols][rows]
    positions += [P31 % cols, (P32 // 4) % cols, cols // 2]           # the columns of the operand's own element 2^31 and byte 2^32
    runs = column_runs(cols, positions)
    taken = {c for c0, w in runs for c in range(c0, c0 + w)}
    plain = [(c0 + w + 40, 8) for c0, w in runs[::3] if c0 + w + 48 <= cols and not taken & set(range(c0 + w + 40, c0 + w + 48))]
    inputs = [(c0, w, specials((rows, w), f32, seed + k)) for k, (c0, w) in enumerate(runs)]
    inputs += [(c0, w, np.stack([generated(oracle, seed, r * cols + c0, w) for r in range(rows)])) for c0, w in plain]
    buf = lib.uniform_f32(rows * cols, seed, 0.0, 1.0)
    a = view(lib, buf, f32, (rows, cols))
    for c0, w, x in inputs[:len(runs)]:
        for r in range(rows):
            lib.upload(buf.base_ptr + (r * cols + c0) * 4, x[r])
    for descending in (False, True):
        vals = lib.sort(a, 0, descending)
        for c0, w, x in inputs:
            got = np.stack([window(lib, vals, r * cols + c0, w) for r in range(rows)])
            assert got.tobytes() == sort_reference(x, 0, descending)[0].tobytes(), (name, descending, c0)
        del vals


def test_sort_columns_of_257(smhip, oracle):
    """S3: f32 (257, 8 355 984) along axis 0, values: ROW | COPY, the skinny transposed copies (cols, 257) in and out.
    Peak 32 GiB: operand 8, result 8, staged operand 8, staged values 8."""
    sort_columns(smhip, oracle, "S3", 44)


def test_sort_columns_of_3(smhip, oracle):
    """S3b: f32 (3, 715 829 250) along axis 0, values: ROW | COPY, record-shaped copies (cols, 3).  Peak 32 GiB as S3."""
    sort_columns(smhip, oracle, "S3b", 45)


# ------------------------------------------------------------------------------------------------------ take
def take_call(lib, case, mode, a_ptr, di, out):
    """The C ABI with the case's own strides and a flag word that holds garbage -> the flag after the call."""
    flag = flag_word(lib)
    rc = lib.take_raw(sma.INDEX_MODES[mode], sma.DTYPES[case["dtype"]], a_ptr, case["a_strides"], case["R"], di.ptr, case["idx_strides"], case["out"],
                      case["axis"], out.ptr, flag.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    return int(flag.numpy()[0])


def test_take_rows_of_a_table(smhip, oracle):
    """T1: 4096 rows of the (2^21 + 5, 1024) f32 table, and of the same buffer as int64 (2^21 + 5, 512): ROWS, once per mode;
    under clip and wrap also ids far outside the axis; under checked one bad id raises.  Peak 8 GiB."""
    lib, seed = smhip, 51
    buf = lib.uniform_f32(ROWS * COLS, seed, 0.0, 1.0)
    rng = np.random.default_rng(seed)
    far = [ROWS, ROWS + P32, -ROWS - 1, -P32, I64_MIN, I64_MAX]
    for name in ("T1", "T1_i64"):
        case = planned(lib, name)
        n, I = case["out"]
        out = lib.empty((n, I), case["dtype"])
        for mode in MODES:
            ids = i64(BOUNDARY_ROWS, far if mode != "checked" else [], rng.integers(-ROWS, ROWS, size=n))[:n]
            di = lib.to_device(ids)
            assert take_call(lib, case, mode, buf.base_ptr, di, out) == 0
            pos, bad = take_normalise(ids, ROWS, mode)
            assert not bad
            uniq, table = rows_table(oracle, seed, pos, COLS)
            assert out.numpy().tobytes() == table[np.searchsorted(uniq, pos)].tobytes(), (name, mode)
        del out
    a = view(lib, buf, f32, (ROWS, COLS))
    ids = rng.integers(-ROWS, ROWS, size=lc.T1_IDS).astype(np.int64)
    ids[1234] = ROWS
    di = lib.to_device(ids)
    with pytest.raises(IndexError):
        lib.take(a, di, 0, mode="checked")


def test_take_along_the_rows_of_a_table(smhip, oracle):
    """T2: take_along_axis of the (2^21 + 5, 1024) table with an (8, 1024) index array along axis 0: DIRECT, an element-granular
    gather whose source offsets pass element 2^31.  Peak 8 GiB."""
    lib, seed = smhip, 52
    case = planned(lib, "T2")
    buf = lib.uniform_f32(ROWS * COLS, seed, 0.0, 1.0)
    rng = np.random.default_rng(seed)
    pool = i64(BOUNDARY_ROWS, rng.integers(-ROWS, ROWS, size=55))
    idx = pool[rng.integers(0, pool.size, size=(8, COLS))]
    idx[:, :9] = np.array(BOUNDARY_ROWS, np.int64)[(np.arange(9)[None, :] + np.arange(8)[:, None]) % 9]   # every boundary row on every j
    first = idx
    out = lib.empty((8, COLS), f32)
    for k, mode in enumerate(MODES):
        idx = np.ascontiguousarray(np.roll(first, 5 * k, axis=1))   # other picks in every mode: `out` keeps nothing a later mode could pass on
        di = lib.to_device(idx)
        assert take_call(lib, case, mode, buf.base_ptr, di, out) == 0
        pos, bad = take_normalise(idx, ROWS, mode)
        assert not bad
        uniq, table = rows_table(oracle, seed, pos, COLS)
        want = table[np.searchsorted(uniq, pos), np.arange(COLS)[None, :]]
        assert out.numpy().tobytes() == np.ascontiguousarray(want).tobytes(), mode
    a = view(lib, buf, f32, (ROWS, COLS))
    assert lib.take_along_axis(a, di, 0).numpy().tobytes() == np.ascontiguousarray(want).tobytes()   # wrap and checked agree on valid indices


def test_take_along_lines_of_1000(smhip, oracle):
    """T3: take_along_axis of f32 (2 147 500, 1000) along its lines, one index line shared by all (stride 0): LINE, eight
    lines staged per workgroup.  The result passes element 2^31.  Peak 16 GiB: operand 8, result 8."""
    lib, seed = smhip, 53
    case = planned(lib, "T3")
    L, R = lc.LINES, lc.LINE
    buf = lib.uniform_f32(L * R, seed, 0.0, 1.0)
    rng = np.random.default_rng(seed)
    idx = rng.integers(-R, R, size=R).astype(np.int64)
    idx[:4] = [0, R - 1, -1, -R]
    first = idx
    out = lib.empty((L, R), f32)
    lines = boundary_lines(L, R, (4,))
    rows = {line: generated(oracle, seed, line * R, R) for line in lines}
    for k, mode in enumerate(MODES):
        idx = np.roll(first, 7 * k)   # other picks in every mode: an entry left unwritten would show the earlier mode's bytes
        di = lib.to_device(idx)
        assert take_call(lib, case, mode, buf.base_ptr, di, out) == 0
        pos, bad = take_normalise(idx, R, mode)
        assert not bad
        for line in lines:
            assert window(lib, out, line * R, R).tobytes() == rows[line][pos].tobytes(), (mode, line)


def wide_windows():
    """Rows of a (WIDE_ROWS, 1031) array at entry 0, across entry 2^32 and at the end: (first row, rows)."""
    k = P32 // lc.WIDE_COLS
    return ((0, 4), (k - 2, 5), (lc.WIDE_ROWS - 4, 4))


def test_take_more_than_2p32_entries(smhip):
    """T4: out[j, i] = a[idx[i], i] over (4 165 924, 1031) from a (7, 1031) table: DIRECT with 2^32 + 100 348 entries, so the flat
    entry counter passes 2^32 while its divisor is 1031.  Peak 16 GiB: the result."""
    lib, seed = smhip, 54
    case = planned(lib, "T4")
    W, R = lc.WIDE_COLS, lc.WIDE_R
    a = specials((R, W), f32, seed)
    rng = np.random.default_rng(seed)
    idx = rng.integers(-R, R, size=W).astype(np.int64)
    idx[:4] = [0, R - 1, -1, -R]
    da, first = lib.to_device(a), idx
    out = lib.empty((lc.WIDE_ROWS * W,), f32)
    for k, mode in enumerate(MODES):
        idx = np.roll(first, 7 * k)   # other picks in every mode: an entry left unwritten would show the earlier mode's bytes
        di = lib.to_device(idx)
        assert take_call(lib, case, mode, da.ptr, di, out) == 0
        pos, bad = take_normalise(idx, R, mode)
        assert not bad
        line = a[pos, np.arange(W)]
        for row0, n in wide_windows():
            assert window(lib, out, row0 * W, n * W).tobytes() == np.tile(line, n).tobytes(), (mode, row0)


def flat_ids(rng, count, extra=()):
    return i64(FLAT_VALID, list(extra), rng.integers(-lc.FLAT, lc.FLAT, size=count))[:count]


def test_take_from_a_flat_axis_past_2p31(smhip, oracle):
    """T5: 4096 picks from a flat f32 array of 2^31 + 4099: pick() clamps, wraps and checks against an R that does not fit 32
    bits.  Every valid form in all three modes; under checked each bad index alone sets the flag (2^32 is out of range here).
    Peak 8 GiB."""
    lib, seed = smhip, 55
    case = planned(lib, "T5")
    R = lc.FLAT
    buf = lib.uniform_f32(R, seed, 0.0, 1.0)
    rng = np.random.default_rng(seed)
    ids = flat_ids(rng, lc.T1_IDS)
    out = lib.empty((lc.T1_IDS,), f32)
    element = {}

    def expected(pos):
        for p in pos.tolist():
            if p not in element:
                element[p] = generated(oracle, seed, p, 1)[0]
        return np.array([element[p] for p in pos.tolist()], f32)

    for k, mode in enumerate(MODES):
        use = np.roll(ids, 11 * k)   # another order in every mode, so that no mode can pass on what the one before left in `out`
        di = lib.to_device(use)
        assert take_call(lib, case, mode, buf.base_ptr, di, out) == 0
        pos, bad = take_normalise(use, R, mode)
        assert not bad
        assert out.numpy().tobytes() == expected(pos).tobytes(), mode
    for wrong in FLAT_BAD:
        ids2 = ids.copy()
        ids2[17] = wrong
        d2 = lib.to_device(ids2)
        assert take_call(lib, case, "checked", buf.base_ptr, d2, out) == 1, wrong
        pos, bad = take_normalise(ids2, R, "checked")   # the clamped element is written
        assert bad and out.numpy().tobytes() == expected(pos).tobytes(), wrong
        for mode in ("clip", "wrap"):
            assert take_call(lib, case, mode, buf.base_ptr, d2, out) == 0
            assert out.numpy().tobytes() == expected(take_normalise(ids2, R, mode)[0]).tobytes(), (mode, wrong)


# ------------------------------------------------------------------------------------------------------ scatter
def scatter_call(lib, case, kind, mode, target, di, dv):
    """The C ABI with the case's own strides and a flag word that holds garbage -> the flag after the call."""
    flag = flag_word(lib)
    rc = lib.scatter_raw(kind, sma.INDEX_MODES[mode], sma.SCATTER_UNIQUE if case["unique"] else 0, sma.DTYPES[case["dtype"]], target.base_ptr, case["out"],
                         case["axis"], di.ptr, case["idx_strides"], dv.ptr, case["val_strides"], case["J"], flag.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    return int(flag.numpy()[0])


class Whole:
    """The whole target checked on the device.  A truncated offset writes somewhere else, and no sample of rows would see it; so
    S = sum((after - before)^2) over every element, through the three operators test_gpu_parity.py pins at 2^31 + 3 elements
    (contiguous SUB, contiguous MUL, sum), against the same sum over the elements the entries name, which the host forms with
    the same f32 difference and f32 product and adds in fp64.  The bound is test_chain.py::test_chain_sum's for a device fp64 sum
    against a host one, 1e-15 * sum(|terms|); a stray element of a uniform [0, 1) target moves S by about 0.1.
    Holds three buffers of the target's size next to the target."""

    def __init__(self, lib, n, seed):
        self.lib, self.n, self.seed = lib, n, seed
        self.before, self.d, self.q = (lib.empty((n,), f32) for _ in range(3))

    def stray_sum(self, target):
        lib = self.lib
        refill(lib, self.before, self.n, self.seed)
        lib.contiguous(sma.OP_SUB, target, self.before, out=self.d)
        lib.contiguous(sma.OP_MUL, self.d, self.d, out=self.q)
        return lib.sum(self.q)

    def check(self, target, before, after, what):
        """before / after: the elements the entries name, as the host has them."""
        got = self.stray_sum(target)
        assert before.shape == after.shape and before.dtype == after.dtype == f32
        width = before.shape[-1] if before.ndim > 1 else 1
        before, after = before.reshape(-1, width), after.reshape(-1, width)
        terms = []
        for r0 in range(0, before.shape[0], 1 << 16):   # the f32 difference and the f32 product, as the device forms them
            d = after[r0:r0 + (1 << 16)] - before[r0:r0 + (1 << 16)]
            terms += (d * d).astype(np.float64).sum(axis=1).tolist()
        want = math.fsum(terms)
        print(f"whole target {what}: S = {got!r}, want {want!r}, |S - want| / want = {abs(got - want) / max(want, 1e-300):.3g}")
        assert abs(got - want) <= 1e-15 * want + 1e-300, (what, got, want)


def table_scatter(lib, oracle, whole, target, name, kind, mode, idx, values, seed):
    """One call on the (2^21 + 5, 1024) table with idx of shape (J, 1) or (J, 1024) along axis 0, checked against the reference run on
    the compact table of the rows the entries name; the rows next to them must be unchanged, and the whole target agree."""
    case = planned(lib, name)
    assert idx.shape[0] == case["J"] and values.shape == (case["J"], COLS)
    refill(lib, target, ROWS * COLS, seed)
    di, dv = lib.to_device(idx), lib.to_device(values)
    flag = scatter_call(lib, case, kind, mode, target, di, dv)
    pos, ok = scatter_normalise(idx, ROWS, mode)
    assert flag == int((~ok).any()), (name, kind, mode, flag)
    touched, compact = rows_table(oracle, seed, pos[ok], COLS)
    remapped = np.where(ok, np.searchsorted(touched, pos), touched.size)     # a dropped entry stays out of range
    want, _ = scatter_reference(kind, compact, remapped, values, 0, "checked")
    for k, row in enumerate(touched.tolist()):
        assert same(kind, window(lib, target, row * COLS, COLS), want[k]), (name, kind, mode, row)
    near = sorted({r for row in touched.tolist() for r in (row - 1, row + 1) if 0 <= r < ROWS} - set(touched.tolist()))
    for row in near:
        assert window(lib, target, row * COLS, COLS).tobytes() == generated(oracle, seed, row * COLS, COLS).tobytes(), (name, kind, mode, row, "untouched")
    whole.check(target, compact, want, (name, kind, mode))


def table_buffers(lib, seed):
    n = ROWS * COLS
    return Whole(lib, n, seed), lib.empty((n,), f32)


def general_f32(rng, shape):
    return (1e3 * rng.standard_normal(shape)).astype(f32)


@pytest.mark.parametrize("kind", **KINDS)
def test_scatter_distinct_rows(smhip, oracle, kind):
    """C1: 300 distinct rows put into / added to the (2^21 + 5, 1024) table with the promise of distinct ids: ROWS.  Peak 32 GiB:
    the target 8 and the three buffers of the whole-target check."""
    lib, seed = smhip, 61
    whole, target = table_buffers(lib, seed)
    rng = np.random.default_rng(seed)
    others = 1 + rng.permutation(ROWS - 10)[:lc.C1_IDS + 20]                 # rows 1 .. 2^21 - 5, on both sides of byte 2^32
    others = others[~np.isin(others, np.mod(DISTINCT_ROWS, ROWS))][:lc.C1_IDS - 6]
    ids = i64(DISTINCT_ROWS, others).reshape(-1, 1)
    assert np.unique(np.mod(ids, ROWS)).size == lc.C1_IDS
    values = general_f32(rng, (lc.C1_IDS, COLS))
    for mode in MODES:
        # DISTINCT_ROWS names rows 0, 2^21 and 2^21 + 4 by their negative forms only.  Clipped, those would all fall on row 0 and
        # break the promise, so under clip they are counted from the front first: the same three rows are still written
        use = np.where(ids < 0, ids + ROWS, ids) if mode == "clip" else ids
        table_scatter(lib, oracle, whole, target, "C1", kind, mode, use, values, seed)


@pytest.mark.parametrize("kind", **KINDS)
def test_scatter_rows_with_duplicates(smhip, oracle, kind):
    """C2: put / index_add of 3000 rows with duplicates, the boundary rows among them several times: SORTED_ROWS (normalise, sort,
    combine).  Peak 32 GiB as C1."""
    lib, seed = smhip, 62
    whole, target = table_buffers(lib, seed)
    rng = np.random.default_rng(seed)
    pool = i64(BOUNDARY_ROWS, rng.integers(-ROWS, ROWS, size=190))
    ids = i64(BOUNDARY_ROWS * 3, pool[rng.integers(0, pool.size, size=lc.C2_IDS - 27)])
    ids = ids[rng.permutation(ids.size)].reshape(-1, 1)
    values = general_f32(rng, (lc.C2_IDS, COLS))
    for mode in MODES:
        table_scatter(lib, oracle, whole, target, "C2", kind, mode, ids, values, seed)


@pytest.mark.parametrize("kind", **KINDS)
def test_scatter_along_the_rows_of_a_table(smhip, oracle, kind):
    """C3: put_along_axis / scatter_add along axis 0 of the table: an (8, 1024) index array of distinct rows per column with the
    promise (DIRECT), and a (24, 1024) one with duplicates without it (SORTED: 1024 sorted lines of 24 keys).  Peak 32 GiB as C1."""
    lib, seed = smhip, 63
    whole, target = table_buffers(lib, seed)
    rng = np.random.default_rng(seed)
    eight = np.array(DISTINCT_ROWS + [5, (1 << 21) + 3], np.int64)
    unique = np.stack([eight[rng.permutation(8)] for _ in range(COLS)], axis=1)
    for mode in MODES:
        use = np.where(unique < 0, unique + ROWS, unique) if mode == "clip" else unique
        table_scatter(lib, oracle, whole, target, "C3_unique", kind, mode, use, general_f32(rng, (8, COLS)), seed)
    pool = i64(BOUNDARY_ROWS, rng.integers(-ROWS, ROWS, size=7))
    dup = pool[rng.integers(0, pool.size, size=(24, COLS))]
    dup[:9, 0] = BOUNDARY_ROWS
    for mode in MODES:
        table_scatter(lib, oracle, whole, target, "C3", kind, mode, dup, general_f32(rng, (24, COLS)), seed)


@pytest.mark.parametrize("kind", **KINDS)
def test_scatter_into_a_flat_axis_past_2p31(smhip, oracle, kind):
    """C4: put / index_add of 5000 entries into a flat f32 array of 2^31 + 4099: SORTED with a merge (5000 > one tile), int64 keys
    above 2^31 and R itself as the key of a dropped entry.  The valid forms in every mode, duplicates on them; the bad ones under
    checked are dropped and set the flag.  Peak 32 GiB: the target 8 and the three buffers of the whole-target check."""
    lib, seed = smhip, 64
    case = planned(lib, "C4")
    R, J = lc.FLAT, lc.C4_IDS
    whole, target = Whole(lib, R, seed), lib.empty((R,), f32)
    rng = np.random.default_rng(seed)
    pool = i64(FLAT_VALID, rng.integers(-R, R, size=400))
    ids = i64(FLAT_VALID * 3, pool[rng.integers(0, pool.size, size=J - 21)])
    ids = ids[rng.permutation(J)]
    broken = ids.copy()
    broken[[5, 1700, 3300, 4999]] = FLAT_BAD
    values = general_f32(rng, (J,))
    dv = lib.to_device(values)
    for mode, use in [(m, ids) for m in MODES] + [("checked", broken)]:
        refill(lib, target, R, seed)
        di = lib.to_device(use)
        flag = scatter_call(lib, case, kind, mode, target, di, dv)
        pos, ok = scatter_normalise(use, R, mode)
        assert flag == int((~ok).any()) == int(use is broken), (kind, mode, flag)
        touched = np.unique(pos[ok])
        compact = np.array([generated(oracle, seed, p, 1)[0] for p in touched.tolist()], f32)
        remapped = np.where(ok, np.searchsorted(touched, pos), touched.size)
        want, _ = scatter_reference(kind, compact, remapped, values, 0, "checked")
        named = set(touched.tolist())
        for k, p in enumerate(touched.tolist()):
            lo, hi = max(p - 1, 0), min(p + 2, R)
            got, was = window(lib, target, lo, hi - lo), generated(oracle, seed, lo, hi - lo)
            for e in range(lo, hi):
                if e == p:
                    assert same(kind, got[e - lo:e - lo + 1], want[k:k + 1]), (kind, mode, p)
                elif e not in named:
                    assert got[e - lo].tobytes() == was[e - lo].tobytes(), (kind, mode, e, "untouched")
        whole.check(target, compact, want, ("C4", kind, mode, use is broken))


@pytest.fixture(scope="module")
def c5(oracle):
    """C5's entries, and what every line of the target holds before the call at the positions they name: one host pass over the
    generated target, shared by the PUT and the ADD test.  Every line is touched, and the oracle makes windows, not columns, so
    the pass regenerates all 2^31 + 16 352 elements in chunks of 2^16 lines and keeps the 21 columns named (180 MB): 1.0 s on
    16 threads, the longest host step of the file."""
    seed, L, R, J = 65, lc.LINES, lc.LINE, lc.C5_ENTRIES
    rng = np.random.default_rng(seed)
    pool = i64([0, R - 1, -1, -R, 1, -2], rng.integers(-R, R, size=18))   # 24 values, fewer positions
    idx = pool[rng.integers(0, pool.size, size=J)]
    idx[:6] = pool[:6]
    # values are multiples of 2^-24 in [0, 1), as the target's own: every partial sum of a destination is then exact in fp64, so the
    # order of the additions cannot change it and the sum of a destination's values may be formed once for every line
    values = (rng.integers(0, 1 << 24, size=J).astype(np.float64) * 2.0 ** -24).astype(f32)
    pos, ok = scatter_normalise(idx, R, "checked")
    assert ok.all()
    cols = np.unique(pos)
    before = np.empty((L, cols.size), f32)
    step = 1 << 16
    for l0 in range(0, L, step):
        n = min(step, L - l0)
        before[l0:l0 + n] = generated(oracle, seed, l0 * R, n * R).reshape(n, R)[:, cols]
    last = np.array([values[np.flatnonzero(pos == c)[-1]] for c in cols], f32)                  # PUT: the largest j wins
    total = np.array([values[pos == c].astype(np.float64).sum() for c in cols], np.float64)    # ADD: exact, whatever the order
    return dict(seed=seed, idx=idx, values=values, cols=cols, before=before, last=last, total=total)


@pytest.mark.parametrize("kind", **KINDS)
def test_scatter_along_lines_of_1000(smhip, oracle, c5, kind):
    """C5: 1500 entries with duplicates along every line of f32 (2 147 500, 1000), one index line and one value line shared by all
    (stride 0): SORTED, one sorted list combined into 2 147 500 lines -- 3.2 * 10^9 entries walked, the target past element 2^31.
    Every line is touched, so there are no untouched neighbours; the sampled lines are compared with the reference and the whole
    target with the closed form the fixture explains.  Peak 32 GiB: the target 8 and the three buffers of the whole-target check."""
    lib, seed = smhip, c5["seed"]
    case = planned(lib, "C5")
    L, R, J = lc.LINES, lc.LINE, lc.C5_ENTRIES
    whole, target = Whole(lib, L * R, seed), lib.empty((L * R,), f32)
    refill(lib, target, L * R, seed)
    di, dv = lib.to_device(c5["idx"]), lib.to_device(c5["values"])
    assert scatter_call(lib, case, kind, "checked", target, di, dv) == 0
    if kind == PUT:
        after = np.broadcast_to(c5["last"], c5["before"].shape)
    else:
        after = np.empty_like(c5["before"])
        for l0 in range(0, L, 1 << 18):
            after[l0:l0 + (1 << 18)] = (c5["before"][l0:l0 + (1 << 18)].astype(np.float64) + c5["total"]).astype(f32)
    for line in boundary_lines(L, R, (4,)):
        row = generated(oracle, seed, line * R, R).reshape(1, R)
        want, bad = scatter_reference(kind, row, c5["idx"].reshape(1, J), c5["values"].reshape(1, J), 1, "checked")
        assert not bad and same(kind, window(lib, target, line * R, R), want[0]), (kind, line)
        assert want[0, c5["cols"]].tobytes() == np.ascontiguousarray(after[line]).tobytes(), (kind, line, "the closed form")
    whole.check(target, c5["before"], after, ("C5", kind))


@pytest.mark.parametrize("kind", **KINDS)
def test_scatter_more_than_2p32_entries(smhip, oracle, kind):
    """C6: out[o, 0, i] (+)= values[i] over (4 165 924, 1, 1031) with one entry per line: DIRECT with 2^32 + 100 348 entries, the
    flat entry counter passing 2^32 while its divisors are 1031 and 1.  idx alternates 0 and -1 under checked (R = 1: both name
    position 0).  Peak 16 GiB: the target."""
    lib, seed = smhip, 66
    case = planned(lib, "C6")
    W = lc.WIDE_COLS
    n = lc.WIDE_ROWS * W
    target = lib.uniform_f32(n, seed, 0.0, 1.0)
    rng = np.random.default_rng(seed)
    values = general_f32(rng, (W,))
    idx = -(np.arange(W, dtype=np.int64) % 2)
    di, dv = lib.to_device(idx), lib.to_device(values)
    assert scatter_call(lib, case, kind, "checked", target, di, dv) == 0
    for row0, rows in wide_windows():
        want = np.tile(values, rows)
        if kind == ADD:
            want = (generated(oracle, seed, row0 * W, rows * W).astype(np.float64) + want).astype(f32)
        assert same(kind, window(lib, target, row0 * W, rows * W), want), (kind, row0)
