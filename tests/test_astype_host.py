"""astype, host side: the 12 conversions themselves (simplemath_amd/csrc/sm_convert.h, the source the gfx950 kernels inline) compiled
for the CPU and checked over their edge sets, once more under the undefined-behaviour sanitizer, and smhip_convert_plan /
smhip_convert's argument checks -- no device involved."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [np.float32, np.float64, np.int32, np.int64]
PAIRS = [(s, d) for s in TYPES for d in TYPES if s != d]


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def _size(dt):
    return np.dtype(dt).itemsize


def test_conversions_on_host():
    """Each of the 12 functions over every exponent x the edge mantissas x both signs, the values around the integer limits, every
    +-2^p and +-(2^p +- 1), the rounding ties and 200 000 random values per source type, against expectations computed in
    integer arithmetic / long double / the rule on the double value.  The program stops at the first mismatch."""
    from simplemath_amd import build
    exe = build.build_host_programs()["convert_host_check"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"convert_host_check: (\d+) checks .* 0 mismatches", r.stdout)
    assert m and int(m.group(1)) >= 3_000_000, r.stdout


def test_no_out_of_range_cast_is_reachable(tmp_path):
    """The same program as a stand-alone build with -fsanitize=undefined,float-cast-overflow: an out-of-range float -> integer cast (undefined,
    and different on host and device) or a signed overflow would abort it."""
    cxx = os.environ.get("CXX", "g++")
    assert shutil.which(cxx), f"{cxx} not found"
    exe = str(tmp_path / "convert_host_check_ubsan")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           f"-I{os.path.join(ROOT, 'simplemath_amd', 'csrc')}", os.path.join(ROOT, "tests", "cpp", "convert_host_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 mismatches" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_entry_points_are_declared():
    syms = sma.declared_symbols()
    assert "smhip_convert" in syms and "smhip_convert_plan" in syms
    header = open(sma.HEADER).read()
    for name, value in (("NONE", sma.CONVERT_ROUTE_NONE), ("DENSE", sma.CONVERT_ROUTE_DENSE), ("ROWS", sma.CONVERT_ROUTE_ROWS),
                        ("STAGED", sma.CONVERT_ROUTE_STAGED), ("COPY", sma.CONVERT_ROUTE_COPY)):
        assert re.search(rf"SMHIP_CONVERT_ROUTE_{name} = {value}\b", header), name


def _view(base_shape, index):
    """(shape, strides in elements) of base[index] for a dense base of this shape."""
    base = np.empty(base_shape, dtype=np.int8)
    v = index(base)
    return list(v.shape), list(v.strides)


@pytest.mark.parametrize("s,d", PAIRS, ids=lambda t: np.dtype(t).name)
def test_plan_routes_and_bytes(lib, s, d):
    ss, ds = _size(s), _size(d)
    cases = [
        ("dense 1-D", [1000], [1], sma.CONVERT_ROUTE_DENSE),
        ("dense 4-D", [3, 2, 5, 7], [70, 35, 7, 1], sma.CONVERT_ROUTE_DENSE),
        ("one element", [1, 1], [1, 1], sma.CONVERT_ROUTE_DENSE),
        ("whole rows m[2:9]", *_view((16, 128), lambda m: m[2:9]), sma.CONVERT_ROUTE_DENSE),
        ("block m[2:9, 5:77]", *_view((16, 128), lambda m: m[2:9, 5:77]), sma.CONVERT_ROUTE_ROWS),
        ("row broadcast over an outer axis", [9, 77], [0, 1], sma.CONVERT_ROUTE_ROWS),
        ("middle axes swapped", *_view((3, 2, 5, 7), lambda m: m.transpose(0, 2, 1, 3)), sma.CONVERT_ROUTE_ROWS),
        ("transpose", *_view((37, 53), lambda m: m.T), sma.CONVERT_ROUTE_STAGED),
        ("x[::2]", *_view((1001,), lambda x: x[::2]), sma.CONVERT_ROUTE_STAGED),
        ("column broadcast", [5, 7], [1, 0], sma.CONVERT_ROUTE_STAGED),
        ("every element the same", [64], [0], sma.CONVERT_ROUTE_STAGED),
    ]
    for what, shape, strides, want in cases:
        n = int(np.prod(shape))
        route, launches, moved = lib.convert_plan(s, d, shape, strides)
        assert route == want, (what, route)
        per = {sma.CONVERT_ROUTE_DENSE: ss + ds, sma.CONVERT_ROUTE_ROWS: ss + ds, sma.CONVERT_ROUTE_STAGED: 3 * ss + ds}[want]
        assert moved == n * per, (what, moved)
        assert launches == (2 if want == sma.CONVERT_ROUTE_STAGED else 1), (what, launches)


@pytest.mark.parametrize("t", TYPES, ids=lambda t: np.dtype(t).name)
def test_plan_equal_dtypes_is_a_copy(lib, t):
    for shape, strides in (([1000], [1]), ([53, 37], [1, 53]), ([500], [2]), ([9, 77], [0, 1])):
        route, launches, moved = lib.convert_plan(t, t, shape, strides)
        assert route == sma.CONVERT_ROUTE_COPY and launches == 1
        assert moved == int(np.prod(shape)) * 2 * _size(t)


def test_plan_empty_shape(lib):
    assert lib.convert_plan(np.float32, np.int64, [0], [1]) == (sma.CONVERT_ROUTE_NONE, 0, 0)
    assert lib.convert_plan(np.float32, np.int64, [4, 0, 3], [0, 3, 1]) == (sma.CONVERT_ROUTE_NONE, 0, 0)


def test_plan_counts_pieces_in_a_child_process():
    """SMHIP_PIECE_LOG2VEC=12: pieces of 2^12 lane groups.  300 001 elements are 75 000 groups of 4 (a 4-byte result: 19 launches)
    or 150 000 of 2 (an 8-byte result: 37 launches); STAGED adds its copy.  The bytes do not change."""
    code = ("import numpy as np, simplemath_amd as sma\n"
            "lib = sma.load()\n"
            "n = 300001\n"
            "for s, d, want in ((np.float32, np.int32, 19), (np.int32, np.float64, 37), (np.float64, np.float32, 19), (np.int64, np.float64, 37)):\n"
            "    ss, ds = np.dtype(s).itemsize, np.dtype(d).itemsize\n"
            "    assert lib.convert_plan(s, d, [n], [1]) == (sma.CONVERT_ROUTE_DENSE, want, n * (ss + ds)), (s, d, lib.convert_plan(s, d, [n], [1]))\n"
            "    assert lib.convert_plan(s, d, [n], [2]) == (sma.CONVERT_ROUTE_STAGED, want + 1, n * (3 * ss + ds))\n"
            "    assert lib.convert_plan(s, d, [4096 * 2], [1])[1] == 1\n"
            "print('plan ok')\n")
    env = dict(os.environ, SMHIP_PIECE_LOG2VEC="12", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "plan ok" in r.stdout, r.stdout + r.stderr


def test_plan_splits_above_256_mib_on_the_wider_side(lib):
    n = (1 << 28) + 4
    assert lib.convert_plan(np.float32, np.int32, [n], [1])[1] == 5       # 1 GiB each side: four pieces of 256 MiB and a rest
    assert lib.convert_plan(np.float32, np.float64, [n], [1])[1] == 9     # 2 GiB on the wider side
    assert lib.convert_plan(np.int64, np.float32, [n], [1])[1] == 9
    assert lib.convert_plan(np.int64, np.float64, [n], [1])[1] == 9
    assert lib.convert_plan(np.float32, np.int32, [1 << 26], [1])[1] == 1  # 256 MiB: one launch


def test_argument_validation_needs_no_gpu(lib):
    f32, f64, i32, i64 = sma.F32, sma.F64, sma.I32, sma.I64
    bad = [
        (9, f32, [1], [4]),            # src dtype
        (f32, -1, [1], [4]),           # dst dtype
        (f32, 4, [1], [4]),            # I8: a dot-product type, not an element type
        (f32, i64, [1] * 7, [2] * 7),  # ndim > MAX_NDIM
        (f32, i64, [1], [-4]),         # negative extent
        (f32, i64, [-1], [4]),         # negative stride
    ]
    for s, d, strides, shape in bad:
        assert lib.convert_raw(s, d, 4096, strides, shape, 1 << 20) == sma.ERR_INVALID, (s, d, strides, shape)
        with pytest.raises(sma.SmhipError):
            lib.convert_plan(s, d, shape, strides)
    assert lib.convert_raw(f32, i64, 4096, None, None, 1 << 20) == sma.ERR_INVALID   # null shape / strides (ndim 0)
    assert lib.convert_raw(f32, i64, 0, [1], [4], 1 << 20) == sma.ERR_INVALID        # null operand
    assert lib.convert_raw(f32, i64, 4096, [1], [4], 0) == sma.ERR_INVALID           # null result
    assert lib.convert_raw(f32, i64, 0, [1], [0], 0) == 0                            # an empty shape is a no-op
    assert lib.convert_raw(f32, f32, 0, [1], [0], 0) == 0
    # any overlap of `out` with the operand's span, out == a included: rejected before anything is launched
    assert lib.convert_raw(f32, i32, 4096, [1], [64], 4096) == sma.ERR_INVALID
    assert lib.convert_raw(f32, f64, 4096, [1], [64], 4096 + 252) == sma.ERR_INVALID
    assert lib.convert_raw(f64, f32, 4096, [1], [64], 4096 - 252) == sma.ERR_INVALID
    assert lib.convert_raw(i32, i32, 4096, [1], [64], 4096) == sma.ERR_INVALID
    assert lib.convert_raw(i32, i64, 4096, [2], [64], 4096 + 4 * 126) == sma.ERR_INVALID  # the last element of a stepped view
    assert b"overlaps" in lib.c.smhip_last_error()


def test_python_surface_refuses_other_types(lib):
    class Fake:  # enough of a DeviceArray for the checks that come before any device is touched
        def __init__(self, dtype, shape):
            self.dtype, self.shape, self.strides, self.ndim, self.size = np.dtype(dtype), tuple(shape), (1,), len(shape), int(np.prod(shape))

        def is_dense(self):
            return True

    a = Fake(np.float32, (8,))
    for bad in (np.int8, np.uint32, np.float16, np.bool_, "complex64"):
        with pytest.raises(TypeError):
            lib.astype(a, bad)
        with pytest.raises(TypeError):
            lib.convert_plan(np.float32, bad, [8], [1])
    with pytest.raises(TypeError):
        lib.astype(Fake(np.int16, (8,)), np.float32)
    with pytest.raises(TypeError):
        lib.astype(a, np.int64, out=Fake(np.int32, (8,)))      # out of another dtype
    with pytest.raises(ValueError):
        lib.astype(a, np.int64, out=Fake(np.int64, (9,)))      # out of another shape
