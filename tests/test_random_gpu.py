"""smhip_random on the device against the CPU model (tests/random_model.py): every kind and element type bit for bit -- the normals
within 5 ULP of the model's fp64 value -- at the sizes around the lane's unit and the workgroup, at unaligned starts, across the carry
of the block number, as a sequence of calls, on either queue, with parameters, as permutation / shuffle, and past 2^32 elements."""
import weakref

import numpy as np
import pytest

import simplemath_amd as sma
from tests import random_model as rm

pytestmark = pytest.mark.gpu

SEED, STREAM = 0x0123456789ABCDEF, 0
SIZES = [0, 1, 3, 4, 5, 7, 8, 1023, 1024, 1025, 65537]
CANARIES = 8
KIND_NAMES = {v: k for k, v in rm.KINDS.items()}
PAIR_IDS = [f"{KIND_NAMES[kind]}-{dt.name}" for kind, dt in rm.PAIRS]
CANARY = {rm.F32: np.float32(-12345.5), rm.F64: np.float64(-12345.5), rm.I32: np.int32(-1234567), rm.I64: np.int64(-1234567890123)}


@pytest.fixture(scope="module")
def lib(smhip):
    smhip.set_device(0)
    return smhip


_model_cache = {}


def model(kind, dt, n, seed=SEED, stream=STREAM, offset=0, params=None):
    """The model's first n elements of a call; element i does not depend on n, so the longest call is computed once and shared."""
    key = (kind, np.dtype(dt), seed, stream, offset, params)
    if key not in _model_cache or _model_cache[key].size < n:
        full = rm.draw(kind, dt, seed, stream, offset, max(n, SIZES[-1]), params)
        full.setflags(write=False)
        _model_cache[key] = full
    return _model_cache[key][:n]


def raw_call(lib, kind, dt, n, seed=SEED, stream=STREAM, offset=0, params=None, start=0):
    """smhip_random into elements [start, start + n) of a buffer of start + n + CANARIES canaries -> (the n results, are all the
    canaries before and after untouched)."""
    dt = np.dtype(dt)
    total = start + n + CANARIES
    buf = lib.to_device(np.full(total, CANARY[dt], dtype=dt))
    params = rm.DEFAULT_PARAMS[kind] if params is None else params
    rc = lib.random_raw(kind, sma.DTYPES[dt], buf.base_ptr + start * dt.itemsize, n, seed, stream, offset, None if kind == rm.BITS else params)
    assert rc == 0, lib.c.smhip_last_error()
    host = buf.numpy()
    rest = np.concatenate([host[:start], host[start + n:]])
    return host[start:start + n], bool((rest == CANARY[dt]).all())


def same(kind, dt, got, want):
    """Bit for bit; NORMAL: within 5 ULP of the model's fp64 value, and exactly 0 where that is 0."""
    if kind == rm.NORMAL:
        if got.size == 0:
            return True
        err = rm.ulp_error(got, want, dt)
        return bool(err.max() <= rm.NORMAL_ULPS)
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("kind,dt", rm.PAIRS, ids=PAIR_IDS)
def test_sizes(lib, kind, dt):
    worst = 0.0
    for n in SIZES:
        got, clean = raw_call(lib, kind, dt, n)
        assert clean, f"n = {n}: an element outside [0, n) was written"
        want = model(kind, dt, n)
        if kind == rm.NORMAL and n:
            worst = max(worst, float(rm.ulp_error(got, want, dt).max()))
        assert same(kind, dt, got, want), (n, got[:8], want[:8])
    if kind == rm.NORMAL:
        print(f"normal {dt}: at most {worst:.3f} ULP from the fp64 model")


@pytest.mark.parametrize("dt,kinds", [(rm.F32, (rm.UNIFORM, rm.NORMAL, rm.BERNOULLI)), (rm.I32, (rm.BITS, rm.INTEGERS)), (rm.F64, (rm.UNIFORM, rm.NORMAL, rm.BERNOULLI))],
                         ids=["float32", "int32", "float64"])
def test_unaligned_start_keeps_the_values(lib, dt, kinds):
    for kind in kinds:
        for n in (5, 1025):
            aligned, _ = raw_call(lib, kind, dt, n)
            assert same(kind, dt, aligned, model(kind, dt, n))
            for start in (1, 2, 3):
                got, clean = raw_call(lib, kind, dt, n, start=start)
                assert clean, (kind, n, start)
                assert got.tobytes() == aligned.tobytes(), (kind, n, start)


@pytest.mark.parametrize("kind,dt", rm.PAIRS, ids=PAIR_IDS)
def test_block_number_carries_and_streams_differ(lib, kind, dt):
    offset = 2 ** 32 - 2
    got, clean = raw_call(lib, kind, dt, 16, offset=offset)
    assert clean and same(kind, dt, got, rm.draw(kind, dt, SEED, STREAM, offset, 16))
    stream = 0x100000005
    other, clean = raw_call(lib, kind, dt, 16, stream=stream)
    zero, _ = raw_call(lib, kind, dt, 16)
    assert clean and same(kind, dt, other, rm.draw(kind, dt, SEED, stream, 0, 16))
    if kind != rm.BERNOULLI:  # (sixteen coin tosses may agree)
        assert other.tobytes() != zero.tobytes()


def test_calls_continue_each_other(lib):
    g, h = lib.generator(SEED), lib.generator(SEED)
    a, b = g.uniform((1024,)), g.uniform((1024,))
    whole = h.uniform((2048,))
    assert g.offset == h.offset == 512
    assert np.concatenate([a.numpy(), b.numpy()]).tobytes() == whole.numpy().tobytes() == model(rm.UNIFORM, rm.F32, 2048).tobytes()
    g = lib.generator(SEED)
    five, four = g.uniform((5,)), g.uniform((4,))
    assert g.offset == 3
    assert five.numpy().tobytes() == rm.draw(rm.UNIFORM, rm.F32, SEED, 0, 0, 5).tobytes()
    assert four.numpy().tobytes() == rm.draw(rm.UNIFORM, rm.F32, SEED, 0, 2, 4).tobytes()
    g.seek(0)
    assert g.uniform((5,)).numpy().tobytes() == five.numpy().tobytes()


def test_either_queue_gives_the_same_bytes(lib):
    """Independent operators of 1 MiB and more alternate between the library's two queues: of three calls into three fresh buffers
    at least one takes the second queue.  All of them, and a repeat into the first buffer, hold the same bytes."""
    n = (1 << 19) + 3
    outs = [lib.empty((n,), np.float32) for _ in range(3)]
    lib.synchronize()
    before = lib.queue_stats()[1]
    for out in outs:
        lib.generator(SEED).normal(out=out)
    assert lib.queue_stats()[1] >= before + 2, "the calls did not alternate between the queues"
    first = outs[0].numpy()
    assert all(o.numpy().tobytes() == first.tobytes() for o in outs[1:])
    lib.generator(SEED).normal(out=outs[0])
    assert outs[0].numpy().tobytes() == first.tobytes()
    assert same(rm.NORMAL, rm.F32, first[:4096], rm.draw(rm.NORMAL, rm.F32, SEED, 0, 0, n, i1=4096))
    assert same(rm.NORMAL, rm.F32, first[-4096:], rm.draw(rm.NORMAL, rm.F32, SEED, 0, 0, n, i0=n - 4096))


def test_parameters(lib):
    n = 4099
    g = lib.generator(SEED)
    u01 = g.uniform((n,)).numpy()
    g.seek(0)
    u = g.uniform((n,), -1.0, 1.0).numpy()
    t = u01 * np.float32(2.0)                       # lo + u * span, two roundings in f32
    assert u.tobytes() == (np.float32(-1.0) + t).tobytes() and u.min() >= -1.0 and u.max() < 1.0
    assert u.tobytes() == rm.draw(rm.UNIFORM, rm.F32, SEED, 0, 0, n, params=(-1.0, 1.0)).tobytes()
    for dt, mean, std in ((np.float32, 0.25, 0.02), (np.float64, -3.0, 1.5)):
        g.seek(7)
        z = g.normal((n,), dtype=dt).numpy()
        g.seek(7)
        scaled = g.normal((n,), mean, std, dtype=dt).numpy()
        t = dt(std) * z                             # mean + std * z from the standard call's own z: exact, no tolerance
        assert scaled.tobytes() == (dt(mean) + t).tobytes()
    for dt in (np.float32, np.float64, np.int32, np.int64):
        assert (g.bernoulli(0.0, (n,), dtype=dt).numpy() == 0).all() and (g.bernoulli(1.0, (n,), dtype=dt).numpy() == 1).all()
    for dt, lo in ((np.int32, -2 ** 31), (np.int32, 2 ** 31 - 1), (np.int64, -2 ** 53), (np.int64, 2 ** 53 - 1)):
        assert (g.integers(lo, lo + 1, (n,), dtype=dt).numpy() == lo).all()
    g.seek(11)
    wide = g.integers(-2 ** 31, 2 ** 31, (n,), dtype=np.int32).numpy()
    assert wide.tobytes() == rm.draw(rm.INTEGERS, rm.I32, SEED, 0, 11, n, params=(-2 ** 31, 2 ** 31)).tobytes()
    assert wide.min() < -2 ** 30 and wide.max() > 2 ** 30
    g.seek(11)
    wide64 = g.integers(-5, 2 ** 32 - 5, (n,)).numpy()
    assert wide64.dtype == np.int64 and wide64.tobytes() == rm.draw(rm.INTEGERS, rm.I64, SEED, 0, 11, n, params=(-5, 2 ** 32 - 5)).tobytes()
    # out=: in place into a dense slice of a larger array, the generator advancing as for a new array
    big = lib.full((3, 1001), 7.0, np.float32)
    row = sma.DeviceArray(lib, big.base_ptr, big.dtype, (1001,), (1,), 1001, big._owner)
    g.seek(0)
    assert g.uniform(out=row) is row and g.offset == 251
    host = big.numpy()
    assert host[1].tobytes() == model(rm.UNIFORM, rm.F32, 1001).tobytes() and (host[0] == 7.0).all() and (host[2] == 7.0).all()


def test_permutation_and_shuffle(lib):
    g = lib.generator(SEED)
    perm = g.permutation(1000).numpy()
    assert g.offset == 500 and perm.dtype == np.int64
    assert np.array_equal(np.sort(perm), np.arange(1000))
    keys = rm.draw(rm.BITS, rm.I64, SEED, 0, 0, 1000)
    assert np.array_equal(perm, np.argsort(keys, kind="stable"))
    x = lib.generator(5).uniform((1000, 7))
    g.seek(0)
    batch = g.shuffle(x, 0).numpy()
    assert batch.tobytes() == x.numpy()[perm].tobytes()
    wide = lib.generator(5).uniform((7, 1000))
    g.seek(0)
    cols = g.shuffle(wide, 1).numpy()
    assert cols.tobytes() == wide.numpy()[:, perm].tobytes()


@pytest.fixture
def device_memory(lib, monkeypatch, request):
    """Every device block the test allocates through the binding is handed back when it ends, passed or failed, and the pool is
    trimmed (tests/test_past_2p31_gpu.py's fixture)."""
    owners = []
    init = sma._Owner.__init__

    def recording(self, lib_, ptr):
        init(self, lib_, ptr)
        owners.append(weakref.ref(self))

    monkeypatch.setattr(sma._Owner, "__init__", recording)
    yield
    for ref in owners:
        owner = ref()
        if owner is not None and owner.ptr:
            lib.free(owner.ptr)
            owner.ptr = 0
    in_use, cached = lib.pool_stats()
    print(f"device memory of {request.node.name}: the pool held {(in_use + cached) / 2 ** 30:.2f} GiB at most, {in_use / 2 ** 30:.2f} GiB still in use")
    lib.pool_trim()


def test_past_2p32_elements(lib, device_memory):
    """One f32 uniform call of 2^32 + 5 elements (16 GiB and 20 bytes; peak device memory: that): element indices and byte offsets
    past 2^32 inside one launch.  Nothing large is downloaded: the windows at the start, around element 2^31 (byte 2^33), around
    element 2^32 to the end, and the canaries behind it, against the model's windows of the same call."""
    n = 2 ** 32 + 5
    buf = lib.empty((n + CANARIES,), np.float32)
    canaries = np.full(CANARIES, CANARY[rm.F32], dtype=np.float32)
    lib.upload(buf.base_ptr + n * 4, canaries)
    out = sma.DeviceArray(lib, buf.base_ptr, np.float32, (n,), (1,), 0, buf._owner)
    g = lib.generator(SEED)
    g.uniform(out=out)
    assert g.offset == 2 ** 30 + 2

    def window(first, count):
        h = np.empty(count, np.float32)
        lib.download(h, buf.base_ptr + first * 4)
        return h

    for i0, i1 in ((0, 64), (2 ** 31 - 32, 2 ** 31 + 32), (2 ** 32 - 32, 2 ** 32 + 5)):
        assert window(i0, i1 - i0).tobytes() == rm.draw(rm.UNIFORM, rm.F32, SEED, 0, 0, n, i0=i0, i1=i1).tobytes(), (i0, i1)
    assert window(n, CANARIES).tobytes() == canaries.tobytes()
