"""The surface fuzzer (tests/cpp/fuzz_surface.cpp) without a device: its generator and host model, tests/cpp/surface_model.h, built
alone with the address and undefined-behaviour sanitizers (surface_model_host).

(a) The coverage of the GPU test is decided here: with its seeds and its case count every row of the table -- statement kinds,
    destination forms, aliasing relations, size classes, the chain-cutting limits, leaf forms -- is reached at least 5 times, and at
    least 99 % of the float elements a run compares are finite in the model.
(b) The model is pinned before it is trusted as a reference: the statements of a few dozen cases are replayed in numpy, which
    carries its own truncating division and wrapping integer power, and the final pools are bit-identical; the integer power is
    checked against the oracle as well."""
import functools
import json
import re
import subprocess

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

SEEDS = (20261, 20262)   # the seeds of tests/test_fuzz_surface_gpu.py
CASES = 96               # ... and its case count: the smallest at which both seeds pass (a) is 48; doubled
REPLAYED = 48            # cases replayed in numpy, of every type and size class
SAN = re.compile(r"AddressSanitizer|LeakSanitizer|runtime error|UndefinedBehaviorSanitizer")


def _exe():
    from simplemath_amd import build
    return build.build_host_programs()["surface_model_host"]


@functools.lru_cache(maxsize=None)
def planned(seed, cases=CASES):
    """The coverage table of `cases` cases of `seed`, as {row: count}, and the (finite, compared) float element counts."""
    r = subprocess.run([_exe(), "--plan-only", "--seed", str(seed), "--cases", str(cases)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not SAN.search(r.stdout + r.stderr), r.stderr[-4000:]
    assert f"surface_model ok seed {seed}" in r.stdout
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"^  (.+): (\d+)$", r.stdout, re.M)}
    m = re.search(r"^finite: (\d+) of (\d+) ", r.stdout, re.M)
    return rows, (int(m.group(1)), int(m.group(2))), table_lines(r.stdout)


def table_lines(stdout):
    return [line for line in stdout.splitlines() if line.startswith("  ") or line.startswith("coverage:") or line.startswith("finite:")]


@pytest.mark.parametrize("seed", SEEDS)
def test_every_row_of_the_table_is_reached(seed):
    rows, _, _ = planned(seed)
    assert len(rows) >= 60, sorted(rows)
    thin = {k: n for k, n in rows.items() if n < 5}
    assert not thin, thin


@pytest.mark.parametrize("seed", SEEDS)
def test_the_compared_floats_are_finite(seed):
    _, (finite, compared), _ = planned(seed)
    assert compared > 0 and finite * 100 >= compared * 99, (finite, compared)


def test_the_program_depends_on_seed_and_case_alone(tmp_path):
    def dump(name, *args):
        path = tmp_path / name
        r = subprocess.run([_exe(), "--dump", str(path), *args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not SAN.search(r.stderr), r.stderr[-4000:]
        return json.loads(path.read_text())
    whole = dump("whole.json", "--seed", "7", "--cases", "8")
    alone = dump("alone.json", "--seed", "7", "--case", "5")
    other = dump("other.json", "--seed", "8", "--case", "5")
    assert len(whole) == 8 and alone == [whole[5]] and other != alone


# ---- (b) the replay in numpy
DT = (np.float32, np.float64, np.int32, np.int64)
UT = (np.uint32, np.uint64, np.uint32, np.uint64)
(BIRTH_ONES, BIRTH_ZEROS, BIRTH_LIST, BIRTH_ADOPT, BIRTH_HOST_TINY, BIRTH_HOST_SMALL, VIEW_NEW, EXPR_NEW, ASSIGN, ASSIGN_TRANSPOSE, ASSIGN_SHIFTED,
 DISCARD, SUM_MEMBER, SUM_FREE, WRITE_DATA, WRITE_REF, WRITE_BULK, RESEED, READ_BURST, READ_CDATA, TO_STRING, ASSIGN_WHERE, PUT_ALONG_AXIS, FAMILY_MAX,
 FAMILY_ARGMAX, FAMILY_SORT, FAMILY_CUMMAX, DROP, DROP_RESULT, MOVE, CONTIGUOUS, REPEAT, REFUSED_EXPR, REFUSED_ROW, WRITE_MID, COMPARE) = range(36)
N_LEAF, N_BIN, N_SCAL, N_LSCAL, N_NEG, N_ABS, N_SQRTABS, N_IPOW = range(8)


def from_bits(bits, t):
    return np.array(bits, dtype=np.uint64).astype(UT[t]).view(DT[t])


def trunc_div(a, b):
    """C's integer division as csrc/ops.hip.h defines it everywhere: toward zero, x / 0 = 0, x / -1 = the wrapping negation."""
    a, b = np.broadcast_arrays(a, b)
    plain = (b != 0) & (b != -1)
    d = np.where(plain, b, 1)
    q = a // d                                         # floor
    q = q + (((a - q * d) != 0) & ((a < 0) != (d < 0)))  # ... toward zero
    return np.where(plain, q, np.where(b == 0, 0, np.negative(a))).astype(a.dtype)


def wrapping_power(a, k):
    r = np.ones_like(a)
    for _ in range(k):
        r = r * a
    return r


class Replay:
    def __init__(self, t):
        self.t, self.storages, self.pool = t, [], {}

    def entry(self, spec):
        st, off, shape, strides = self.pool[spec["slot"]]
        if spec["t"]:
            shape, strides = shape[::-1], strides[::-1]
        if spec["sl"]:
            nshape, nstrides = [], []
            for d, (n, s) in enumerate(zip(shape, strides)):
                kind, a, b, step = spec["sl"][d] if d < len(spec["sl"]) else (0, 0, 0, 1)
                if kind == 0:
                    nshape.append(n), nstrides.append(s)
                elif kind == 1:
                    off += a * s
                    nshape.append((b - a + step - 1) // step), nstrides.append(s * step)
                else:
                    off += a * s
            shape, strides = nshape, nstrides
        return st, off, list(shape), list(strides)

    def array(self, e):
        st, off, shape, strides = e
        base = self.storages[st]
        return as_strided(base[off:], shape, [s * base.itemsize for s in strides])

    def born(self, slot, values, shape):
        self.storages.append(np.ascontiguousarray(values).reshape(-1).copy())
        dense = [int(np.prod(shape[i + 1:], dtype=np.int64)) for i in range(len(shape))]
        self.pool[slot] = (len(self.storages) - 1, 0, list(shape), dense)

    def op(self, op, a, b):
        if op == 3 and self.t >= 2:
            return trunc_div(a, b)
        return (np.add, np.subtract, np.multiply, np.divide)[op](a, b)

    def eval(self, expr, at=None):
        n = expr["nodes"][expr["root"] if at is None else at]
        kind = n["kind"]
        if kind == N_LEAF:
            return self.array(self.entry(n["leaf"]))
        a = self.eval(expr, n["a"])
        if kind == N_BIN:
            return self.op(n["op"], a, self.eval(expr, n["b"]))
        if kind == N_SCAL:
            return self.op(n["op"], a, from_bits([n["scalar"]], self.t)[0:1].reshape(()))
        if kind == N_LSCAL:
            return self.op(n["op"], from_bits([n["scalar"]], self.t), a)
        if kind == N_NEG:
            return np.negative(a)
        if kind == N_ABS:
            return np.abs(a)
        if kind == N_SQRTABS:
            return np.sqrt(np.abs(a))
        return wrapping_power(a, n["k"])

    def run(self, s):
        kind, t = s["kind"], self.t
        if kind <= BIRTH_HOST_SMALL:
            self.born(s["slot2"], from_bits(s["values"], t), s["shape"])
        elif kind == VIEW_NEW:
            self.pool[s["slot2"]] = self.entry(s["dst"])
        elif kind == EXPR_NEW:
            v = np.array(self.eval(s["expr"]))
            self.born(s["slot2"], v, v.shape)
        elif kind in (ASSIGN, ASSIGN_SHIFTED):
            v = np.array(self.eval(s["expr"]))  # numpy's meaning: the right-hand side completely, then the store
            self.array(self.entry(s["dst"]))[...] = v
        elif kind == ASSIGN_TRANSPOSE:
            x = self.array(self.pool[s["slot"]])
            x[...] = x.T.copy()
        elif kind == WRITE_DATA:
            st, off, _, _ = self.pool[s["slot"]]
            for i, v in zip(s["at"], from_bits(s["values"], t)):
                self.storages[st][off + i] = v
        elif kind == WRITE_REF:
            st, off, shape, strides = self.pool[s["slot"]]
            nd = len(shape)
            for i, v in enumerate(from_bits(s["values"], t)):
                self.storages[st][off + sum(p * q for p, q in zip(s["at"][i * nd:(i + 1) * nd], strides))] = v
        elif kind in (WRITE_BULK, RESEED):
            st, off, _, _ = self.pool[s["slot"]]
            first = off - s["at"][0] + s["at"][1]
            self.storages[st][first:first + len(s["values"])] = from_bits(s["values"], t)
        elif kind == ASSIGN_WHERE:
            x = self.array(self.entry(s["dst"]))
            x[x > from_bits([s["scalar"]], t)[0]] = from_bits([s["scalar2"]], t)[0]
        elif kind == PUT_ALONG_AXIS:
            x = self.array(self.entry(s["dst"]))
            np.put_along_axis(x, np.array(s["index"], dtype=np.int64).reshape(s["index_shape"]), from_bits([s["scalar"]], t)[0], s["axis"])
        elif kind == DROP:
            del self.pool[s["slot"]]
        elif kind == MOVE:
            self.pool[s["slot2"]] = self.pool.pop(s["slot"])
        elif kind == CONTIGUOUS:
            v = np.array(self.array(self.entry(s["dst"])))
            self.born(s["slot2"], v, v.shape)
        elif kind == WRITE_MID:  # E first, then the write to one of its operands, then the right operand
            left = np.array(self.eval(s["expr"]))
            st, off, _, _ = self.pool[s["slot"]]
            if s["variant"] == 0:
                for i, v in zip(s["at"], from_bits(s["values"], t)):
                    self.storages[st][off + i] = v
            else:
                x = self.array(self.pool[s["slot"]])
                x[x > from_bits([s["scalar"]], t)[0]] = from_bits([s["scalar2"]], t)[0]
            v = self.op(s["op"], left, self.array(self.entry(s["dst"])))
            self.born(s["slot2"], v, v.shape)
        # everything else observes and changes nothing


@functools.lru_cache(maxsize=None)
def dumped(seed, cases):
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dump.json")
        r = subprocess.run([_exe(), "--dump", path, "--seed", str(seed), "--cases", str(cases)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not SAN.search(r.stdout + r.stderr), r.stderr[-4000:]
        with open(path) as f:
            return json.load(f)


def test_the_model_agrees_with_a_replay_in_numpy():
    cases = dumped(SEEDS[0], REPLAYED)
    assert len(cases) == REPLAYED and {c["type"] for c in cases} == {0, 1, 2, 3} and {c["class"] for c in cases} == {"tiny", "small", "mid"}
    compared = 0
    with np.errstate(all="ignore"):
        for c in cases:
            t = c["type"]
            replay = Replay(t)
            for s in c["statements"]:
                replay.run(s)
            assert sorted(replay.pool) == [e["slot"] for e in c["pool"]], (c["case"], sorted(replay.pool))
            for e in c["pool"]:
                got = np.array(replay.array(replay.pool[e["slot"]]))
                want = from_bits(e["bits"], t).reshape(e["shape"])
                assert got.shape == want.shape, (c["case"], e["slot"])
                same = got.view(UT[t]) == want.view(UT[t])
                if t < 2:
                    same |= np.isnan(got) & np.isnan(want)
                if not same.all():
                    i = int(np.flatnonzero(~same.reshape(-1))[0])
                    raise AssertionError(f"seed {c['seed']} case {c['case']} v{e['slot']} element {i}: model {want.reshape(-1)[i]!r}, numpy {got.reshape(-1)[i]!r}")
                compared += got.size
    assert compared > 1_000_000


def test_the_integer_rules_of_the_replay_against_the_oracle():
    """The replay's wrapping power against the oracle's array_scalar POW (the reference's square-and-multiply), and its division
    against C's on the edges: truncation, x / 0 = 0, INT_MIN / -1 = INT_MIN."""
    from oracle import oracle as orc
    orc.build(ref=False)
    o = orc.Oracle()
    rng = np.random.default_rng(5)
    for dt in (np.int32, np.int64):
        info = np.iinfo(dt)
        a = np.concatenate([rng.integers(-9, 10, 300), rng.integers(info.min, info.max, 300, dtype=np.int64 if dt == np.int64 else np.int64),
                            [info.min, info.max, 0, 1, -1, 46341, -46341, 3037000500]]).astype(dt)
        with np.errstate(all="ignore"):
            for k in range(4):
                assert np.array_equal(wrapping_power(a, k), o.array_scalar(orc.POW, a, k)), (dt, k)
            x = np.array([7, -7, 7, -7, info.min, info.min, 5, info.min, info.max, 0], dtype=dt)
            y = np.array([2, 2, -2, -2, -1, 1, 0, 2, -1, 0], dtype=dt)
            want = [3, -3, -3, 3, info.min, info.min, 0, info.min // 2, -info.max, 0]
            assert trunc_div(x, y).tolist() == want, dt
