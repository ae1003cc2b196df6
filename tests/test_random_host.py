"""Random draws, host side: Philox4x32-10 and the maps from words to values (simplemath_amd/csrc/sm_random.h, the source the gfx950
kernels inline) compiled for the CPU and held against the CPU model (tests/random_model.py); the accuracy of the normal's pieces
against long double; once more under the undefined-behaviour sanitizer; smhip_random_blocks and every refusal of smhip_random; and
the statistical sanity of the definition itself, on the model -- no device involved."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import simplemath_amd as sma
from tests import random_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_NAMES = {rm.BITS: "bits", rm.UNIFORM: "uniform", rm.INTEGERS: "integers", rm.BERNOULLI: "bernoulli", rm.NORMAL: "normal"}
TYPE_NAMES = {rm.F32: "f32", rm.F64: "f64", rm.I32: "i32", rm.I64: "i64"}
KNOWN_ANSWERS = ["6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd", "d16cfe09 94fdcceb 5001e420 24126ea1"]
SEED, STREAM, OFFSET = 0x0123456789ABCDEF, 0x100000005, 2 ** 32 - 1  # both halves of the seed nonzero, a stream, the carry


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


@pytest.fixture(scope="module")
def exe():
    from simplemath_amd import build
    return build.build_host_programs()["random_host_check"]


def test_known_answers_from_the_model():
    cases = [((0, 0, 0, 0), (0, 0)), ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))]
    for (ctr, key), want in zip(cases, KNOWN_ANSWERS):
        out = rm.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
        assert " ".join(f"{int(w[0]):08x}" for w in out) == want
    # ... and through (seed, stream, block number)
    w = rm.block_words(0x299F31D0A4093822, 0x0370734413198A2E, 0, 0x85A308D3243F6A88, 0x85A308D3243F6A89)
    assert " ".join(f"{int(x):08x}" for x in w[0]) == KNOWN_ANSWERS[2]


def test_known_answers_from_the_header(exe):
    r = subprocess.run([exe, "kat"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "kat: 0 mismatches" in r.stdout, r.stdout + r.stderr
    assert [line[4:] for line in r.stdout.splitlines() if line.startswith("kat ")] == KNOWN_ANSWERS


def _host_values(exe, n):
    r = subprocess.run([exe, "values", str(SEED), str(STREAM), str(OFFSET), str(n)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        kind, dtype, *bits = line.split()
        got[kind, dtype] = bits
    return got


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_host_program_equals_the_model(exe, n):
    got = _host_values(exe, n)
    assert len(got) == len(rm.PAIRS)
    for kind, dt in rm.PAIRS:
        bits = got[KIND_NAMES[kind], TYPE_NAMES[dt]]
        assert len(bits) == n
        raw = np.array([int(b, 16) for b in bits], dtype=np.uint64).astype(np.uint32 if dt.itemsize == 4 else np.uint64).view(dt)
        want = rm.draw(kind, dt, SEED, STREAM, OFFSET, n)  # the host program's parameters are the model's defaults
        if kind == rm.NORMAL:
            err = rm.ulp_error(raw, want, dt)
            print(KIND_NAMES[kind], dt, "max ULP", err.max())
            assert err.max() <= rm.NORMAL_ULPS
        else:
            assert want.dtype == dt and np.array_equal(want.view(np.uint8), raw.view(np.uint8)), (KIND_NAMES[kind], dt, want, raw)


def _check_accuracy(stdout):
    found = dict((m.group(1), (float(m.group(2)), int(m.group(3)))) for m in re.finditer(r"^(\w+) max_ulp ([0-9.]+|inf) at (\d+)$", stdout, re.M))
    assert sorted(found) == ["cospi_f32", "cospi_f64", "r_f32", "r_f64", "sinpi_f32", "sinpi_f64"], stdout
    for piece, (err, arg) in found.items():
        print(piece, err, "ULP at", arg)
        assert err <= 1.0, (piece, err, arg)
    assert "accuracy: 0 exact-value mismatches" in stdout  # cospi(1/2) == 0, sinpi(0) == 0, r(u1 = 1) == 0


def test_accuracy_of_the_normals_pieces(exe):
    """r(u1), cospi(2t) and sinpi(2t): f32 over all 2^24 inputs, f64 over 2^22 pseudo-random 53-bit inputs and the edge sets, against
    long double (the turn reduced to an octant exactly): <= 1 ULP each, the standard of the in-register exp / log.  Measured: r 0.8514 /
    0.8467, cospi 0.5000 / 0.7832, sinpi 0.5000 / 0.7808 ULP (f32 / f64)."""
    r = subprocess.run([exe, "accuracy"], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    _check_accuracy(r.stdout)


def test_no_undefined_behaviour_is_reachable(tmp_path):
    """The same program as a stand-alone build with -fsanitize=undefined,float-cast-overflow: known answers, the accuracy sweeps and a
    `values` run (every kind and dtype at the carry) with no report."""
    cxx = os.environ.get("CXX", "g++")
    assert shutil.which(cxx), f"{cxx} not found"
    exe = str(tmp_path / "random_host_check_ubsan")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           f"-I{os.path.join(ROOT, 'simplemath_amd', 'csrc')}", os.path.join(ROOT, "tests", "cpp", "random_host_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "kat: 0 mismatches" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    _check_accuracy(r.stdout)
    v = subprocess.run([exe, "values", str(SEED), str(STREAM), str(OFFSET), "9"], capture_output=True, text=True, timeout=60)
    assert v.returncode == 0 and "runtime error" not in v.stderr, v.stdout + v.stderr


def test_entry_points_are_declared():
    syms = sma.declared_symbols()
    assert "smhip_random" in syms and "smhip_random_blocks" in syms
    header = open(sma.HEADER).read()
    for name, value in (("BITS", sma.RANDOM_BITS), ("UNIFORM", sma.RANDOM_UNIFORM), ("INTEGERS", sma.RANDOM_INTEGERS),
                        ("BERNOULLI", sma.RANDOM_BERNOULLI), ("NORMAL", sma.RANDOM_NORMAL)):
        assert re.search(rf"SMHIP_RANDOM_{name} = {value}\b", header), name
        assert getattr(rm, name) == value


def test_blocks(lib):
    for kind, dt in rm.PAIRS:
        per = rm.per_block(kind, dt)
        assert per == (2 if kind == rm.INTEGERS or (dt.itemsize == 8 and kind != rm.BERNOULLI) else 4)
        for n, want in ((0, 0), (1, 1), (4, 4 // per), (5, -(-5 // per))):
            assert lib.random_blocks(kind, dt, n) == want == rm.blocks(kind, dt, n), (kind, dt, n)
    assert lib.random_blocks("integers", np.int32, 5) == 3 and lib.random_blocks("normal", np.float64, 5) == 3
    assert lib.random_blocks("uniform", np.float32, 2 ** 32 + 5) == 2 ** 30 + 2


def test_refusals_need_no_gpu(lib):
    f32, f64, i32, i64 = sma.F32, sma.F64, sma.I32, sma.I64
    B, U, I, P, N = sma.RANDOM_BITS, sma.RANDOM_UNIFORM, sma.RANDOM_INTEGERS, sma.RANDOM_BERNOULLI, sma.RANDOM_NORMAL
    inf, nan = float("inf"), float("nan")
    ptr = 1 << 20  # never dereferenced: every call below is refused before a device is touched
    bad = [
        (5, f32, (0.0, 1.0)), (-1, f32, (0.0, 1.0)),                      # kind
        (U, 4, (0.0, 1.0)), (U, -1, (0.0, 1.0)),                          # dtype
        (U, i32, (0.0, 1.0)), (U, i64, (0.0, 1.0)), (N, i32, (0.0, 1.0)), (N, i64, (0.0, 1.0)),  # float kinds of integer types
        (B, f32, None), (B, f64, None), (I, f32, (0.0, 10.0)), (I, f64, (0.0, 10.0)),            # integer kinds of float types
        (N, f32, (0.0, -1.0)), (N, f64, (0.0, -1e-300)),                  # std < 0
        (N, f32, (nan, 1.0)), (N, f32, (0.0, inf)), (N, f64, (inf, 1.0)), (N, f64, (0.0, nan)),  # non-finite
        (U, f32, (nan, 1.0)), (U, f32, (0.0, inf)), (U, f64, (-inf, 0.0)),
        (U, f32, (1.0, 0.0)), (U, f64, (1.0, 0.5)),                       # hi < lo
        (I, i32, (0.0, 0.0)), (I, i64, (5.0, 5.0)), (I, i64, (5.0, 4.0)),   # R < 1
        (I, i64, (0.0, 2.0 ** 32 + 1)), (I, i64, (-2.0 ** 40, 2.0 ** 40)),  # R > 2^32
        (I, i32, (0.0, 2.0 ** 32)), (I, i32, (-2.0 ** 31 - 1, 0.0)),        # beyond the element type
        (I, i64, (0.5, 10.0)), (I, i32, (0.0, 10.5)), (I, i64, (nan, 10.0)), (I, i64, (0.0, inf)),  # not whole numbers
        (P, f32, (-0.01, 0.0)), (P, i64, (1.01, 0.0)), (P, f64, (nan, 0.0)), (P, i32, (inf, 0.0)),  # p outside [0, 1]
        (U, f32, None), (N, f64, None), (I, i32, None), (P, i64, None),    # null params
    ]
    for kind, dtype, params in bad:
        assert lib.random_raw(kind, dtype, ptr, 16, 1, 0, 0, params) == sma.ERR_INVALID, (kind, dtype, params)
        assert lib.random_raw(kind, dtype, ptr, 0, 1, 0, 0, params) == sma.ERR_INVALID, (kind, dtype, params, "n = 0")
    # offset + blocks passing 2^64
    top = 2 ** 64
    assert lib.random_raw(U, f32, ptr, 5, 1, 0, top - 1, (0.0, 1.0)) == sma.ERR_INVALID  # two blocks
    assert lib.random_raw(U, f64, ptr, 3, 1, 0, top - 1, (0.0, 1.0)) == sma.ERR_INVALID
    assert lib.random_raw(I, i32, ptr, 8, 1, 0, top - 3, (0.0, 10.0)) == sma.ERR_INVALID  # four blocks
    assert b"2^64" in lib.c.smhip_last_error()
    # a null result with n > 0; n == 0 is a no-op that touches no device
    assert lib.random_raw(U, f32, 0, 4, 1, 0, 0, (0.0, 1.0)) == sma.ERR_INVALID
    assert lib.random_raw(U, f32, 0, 0, 1, 0, top - 1, (0.0, 1.0)) == 0
    assert lib.random_raw(B, i64, 0, 0, 1, 0, 0, None) == 0
    assert lib.random_raw(I, i32, 0, 0, 1, 0, 0, (-2.0 ** 31, 2.0 ** 31)) == 0  # the widest ranges are accepted
    assert lib.random_raw(I, i64, 0, 0, 1, 0, 0, (2.0 ** 63 - 2.0 ** 32, 2.0 ** 63)) == 0
    assert lib.random_raw(P, f32, 0, 0, 1, 0, 0, (1.0, 0.0)) == 0 and lib.random_raw(P, f32, 0, 0, 1, 0, 0, (0.0, 0.0)) == 0


def test_python_surface_refuses(lib):
    class Fake:  # enough of a DeviceArray for the checks that come before any device is touched
        def __init__(self, dtype, shape, dense=True):
            self.dtype, self.shape, self.size, self.ptr, self.dense = np.dtype(dtype), tuple(shape), int(np.prod(shape)), 1 << 20, dense

        def is_dense(self):
            return self.dense

    g = lib.generator(7)
    with pytest.raises(TypeError):
        g.uniform(out=Fake(np.int32, (8,)))
    with pytest.raises(TypeError):
        g.normal(out=Fake(np.int64, (8,)))
    with pytest.raises(TypeError):
        g.integers(0, 10, out=Fake(np.float32, (8,)))
    with pytest.raises(TypeError):
        g.bits(out=Fake(np.float64, (8,)))
    with pytest.raises(TypeError):
        g.bernoulli(0.5, out=Fake(np.int16, (8,)))
    with pytest.raises(TypeError):
        g.uniform(dtype=np.float64, out=Fake(np.float32, (8,)))   # out of another dtype
    with pytest.raises(TypeError):
        lib.random_blocks("uniform", np.int32, 4)
    with pytest.raises(ValueError):
        g.uniform(out=Fake(np.float32, (8,), dense=False))
    with pytest.raises(ValueError):
        g.uniform(lo=1.0, hi=0.0, out=Fake(np.float32, (8,)))
    with pytest.raises(ValueError):
        g.normal(std=-1.0, out=Fake(np.float32, (8,)))
    with pytest.raises(ValueError):
        g.integers(0, 2 ** 32 + 1, out=Fake(np.int64, (8,)))
    with pytest.raises(ValueError):
        g.integers(0, 2 ** 53 + 1, out=Fake(np.int64, (8,)))
    with pytest.raises(ValueError):
        g.bernoulli(1.5, out=Fake(np.float32, (8,)))
    assert g.offset == 0  # a refused call does not advance the generator


# ------------------------------------------------------------------------------------------- sanity of the definition, on the model
DRAWS = 1 << 20


def test_uniform_mean():
    u = rm.draw(rm.UNIFORM, np.float32, 1, 0, 0, DRAWS).astype(np.float64)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / DRAWS)


def test_normal_mean_and_variance():
    z = rm.draw(rm.NORMAL, np.float32, 1, 0, 0, DRAWS)
    assert abs(z.mean()) <= 5 / 2 ** 10
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2 / DRAWS)


def test_integers_chi_square():
    k = rm.draw(rm.INTEGERS, np.int32, 1, 0, 0, DRAWS, params=(0, 10))
    assert k.min() == 0 and k.max() == 9
    counts = np.bincount(k, minlength=10)
    chi2 = float(((counts - DRAWS / 10) ** 2 / (DRAWS / 10)).sum())
    print("chi-square on 9 degrees of freedom:", chi2)
    assert chi2 < 33.7  # p = 1e-4
