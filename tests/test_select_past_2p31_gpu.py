"""flatnonzero and select over more than 2^31 elements: an int32 array of 2^31 + 4099 zeros (8 GiB) with a handful of nonzero elements
on both sides of element 2^31 (byte 2^33) and in the last tile.  What this size reaches and the small shapes of test_select_gpu.py
cannot: vector and element indices past 2^31 inside the tile kernels, the int64 positions written out, and a prefix over more than
2^18 tile counts (129 passes of the one-workgroup prefix kernel).

The expectation is written down, not computed: the positions uploaded are the positions that must come back, in ascending order, with
the values uploaded there.  Nothing large is uploaded or downloaded.  Peak device memory: 8 GiB and the tile counts (6 MiB)."""
import weakref

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

P31 = 1 << 31
N = P31 + 4099


@pytest.fixture(autouse=True)
def device_memory(smhip, monkeypatch, request):
    """Every device block the test allocates through the binding is handed back when it ends, passed or failed, and the pool is
    trimmed: a red test must not leave 8 GiB behind for the next one to trip over."""
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
    smhip.pool_trim()


def test_flatnonzero_and_select_past_2p31(smhip):
    lib = smhip
    route, launches, (tiles, tile, threshold, copies) = lib.select_plan("index", np.int32, [N], [1])
    assert (route, launches, copies) == (sma.SELECT_ROUTE_TILES, 3, 0) and tiles == -(-N // tile) and tiles > 1 << 18
    last_tile = (tiles - 1) * tile
    # N - 3 and N - 1 lie behind the last whole 16-byte vector: the kernels read them one by one
    positions = [0, 5, tile - 1, tile, P31 - tile - 1, P31 - 4, P31 - 1, P31, P31 + 1, P31 + 2047, N - 3, N - 1]
    assert positions == sorted(set(positions)) and positions[-1] < N and sum(p >= last_tile for p in positions) >= 3 and N % 4 == 3
    values = np.array([-(k + 1) if k % 2 else k + 1 for k in range(len(positions))], np.int32)   # nonzero, both signs, all different
    x = lib.full((N,), 0, np.int32)
    for p, v in zip(positions, values):
        lib.upload(x.base_ptr + 4 * p, np.array([v], np.int32))
    want = np.array(positions, np.int64)
    assert lib.count_nonzero(x) == len(positions)
    got = lib.flatnonzero(x)
    assert got.shape == (len(positions),) and np.array_equal(got.numpy(), want)
    assert np.array_equal(lib.select(x, x).numpy(), values)
    # a comparison instead of "nonzero": the negative ones, and, through !=, everything but them
    negative = values < 0
    assert np.array_equal(lib.flatnonzero((x, "lt", 0)).numpy(), want[negative])
    assert np.array_equal(lib.select(x, (x, "gt", 0)).numpy(), values[~negative])
    assert lib.count_nonzero((x, "eq", 0)) == N - len(positions)
    # capacity: the first five of the zeros' positions past 2^31 ... are not asked for; the first five nonzero ones are
    out = lib.full((5,), -1, np.int64)
    word = lib.full((1,), -1, np.int64)
    rc = lib.select_raw(sma.SELECT_INDEX, sma.CMP_NONZERO, sma.I32, x.ptr, [1], 0, None, None, [N], 0, None, 0, out.ptr, 5, word.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    assert np.array_equal(out.numpy(), want[:5]) and int(word.numpy()[0]) == len(positions)
