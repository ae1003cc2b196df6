"""Every entry point that declares operand spans to the two-queue dispatcher (csrc/queue_order.h, runtime.hip), raced on the GPU.

Each scenario has one shape.  Everything it uses is warmed up and the device synchronised; then
  1. BALLAST: K_BALLAST dependent in-place chains of STAGES f64 pow stages on W (all ones, so W stays all ones): one queue is
     busy for milliseconds;
  2. a GATE, one tracked copy that ties the slow side to the ballast by a dependency of the OTHER kind than the one under test
     (so the slow side stays behind the ballast even in a library whose tracker misses the kind under test):
       gate_read(X)   copies bytes of X into W's tail -- it writes bytes the ballast used, and the later WRITER of X is behind it;
       gate_write(S)  copies W's head (the f64 ones) into S -- it reads what the ballast wrote, and the later READER of S is behind it;
  3. P, the slow side, behind the gate and therefore milliseconds away;
  4. C, the fast side, issued at once: it conflicts with P on the span X and with nothing else, so without the edge between the
     two it takes the idle queue and runs before P has started;
  5. X is prefilled with a sentinel, and every buffer is compared bit for bit with numpy on the host arrays (the uniform fill with
     the oracle, as the rest of the suite does).
RAW: P writes X, C reads it.  WAR: P reads X (what the gate put there), C overwrites it.  WAW: both write X, C's values stay.
A scenario fails as NOT EXERCISED unless the device stayed busy after the last call returned for at least as long as issuing
steps 1-4 took.  K_BALLAST = 10 chains of STAGES = 14 stages on 96 MiB: see MEASURED below for what that gives on an MI355X.

Scenarios run in a fresh child process per test (an earlier test of the pytest process may have switched the device to one
queue for good); the child refuses to start unless queue_stats() reports two queues.

fill, the uniform fill and the Generator's draw (smhip_random, "random") read nothing: they play P in RAW and C in WAR / WAW only
(behind gate_read a writer is held back by a WAR dependency alone, which is what the WAW scenarios test).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

K_BALLAST = 10
STAGES = 14
W_ELEMS = 12 << 20          # f64: 96 MiB, 192 MiB of operand bytes per ballast chain (tracked: under 224 MiB)
GATE_MAX = 16 << 20
N = 2 << 20                 # elements of the generic buffers: 8 MiB of f32
ROWS, COLS = 512, 4096
MEASURED = """
On an MI355X, K_BALLAST = 10, STAGES = 14, W = 96 MiB (one ballast stage: about 3.3 us to issue, about 37 us on the device):
issuing steps 1-4 took 0.46-0.74 ms per scenario (1.3 ms for a process's very first one), after which the device stayed busy for
4.2-5.3 ms: 6.6 to 10.6 times the issue time (3.3 times in that first one).  The margin is set by the ballast's stage, not by K --
a chain on more than 112 MiB would leave the two-queue range -- so K only sets the length of the window.

Sensitivity: the file run once against libraries built with one piece of queue_order.h's ordering removed (no kernel and no
address differs, so they can only give wrong values).  Red = the scenario failed its bit-for-bit comparison.  The counts below
were measured before the "random" entry joined ENTRIES (18 entries then, 19 now) and have not been measured again.
  RAW loop of dependencies() removed    every "raw:" scenario between two tracked entry points (13 of 18; the 5 with a barrier
                                        operator on one side are ordered by the barrier), every "span: RAW" scenario but the
                                        operator under 1 MiB (a barrier), the operator over 224 MiB; nothing else.
  WAR / WAW block removed               every "war:" and "waw:" scenario between two tracked entry points (13 of 18 each), the
                                        three "span: WAR" scenarios, all six "pool: ... filled again" repetitions and the cut
                                        chains' temporaries (note_scratch asks the same block of dependencies()); nothing else.
  note_scratch returning at once        "pool: WAR, dropped operands' blocks as the temporaries of cut chains"; nothing else.
  queue_barrier not raising floor[0]    (a fourth library, for the scenarios the first three cannot reach) the two "tiny:"
                                        scenarios in which a later tracked operator must wait for the flush of recorded operators.
"tiny: RAW, 25 elements of X read by a recorded operator" is green under all four: the flush is a barrier operator, behind
everything by stream order and one wait; it is here for the value.
"""

GROUPS = ["raw", "war", "waw", "spans_a", "spans_b", "large", "tiny", "pool"]
CHILD_TIMEOUT = {"large": 120}


@pytest.mark.parametrize("group", GROUPS)
def test_queue_order_raced(group, oracle):
    """One child process runs the group's scenarios; each must be right bit for bit AND report that it raced."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), group], capture_output=True, text=True, timeout=CHILD_TIMEOUT.get(group, 90), cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-6000:]}\n{r.stderr[-3000:]}"
    lines = [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("RACE ")]
    assert lines and lines[-1].get("done") == group, r.stdout[-3000:]
    bad = [s for s in lines[:-1] if not (s["ok"] and s["raced"])]
    assert not bad, bad
    assert len(lines) - 1 >= lines[-1]["scenarios"] > 0


# ====================================================================================================== the child process
def _child(group):
    sys.path.insert(0, ROOT)
    import ctypes as C

    import simplemath_amd as sma
    from oracle import oracle as orc
    from simplemath_amd import DeviceArray
    from tests import random_model

    lib = sma.load()
    lib.set_device(0)
    rng = np.random.default_rng(20240 + GROUPS.index(group))
    f32 = np.float32

    def view(arr, dtype, byte_offset, shape, strides=None):
        """A view of arr's allocation: element type, offset in bytes from the allocation's start, shape, strides in elements."""
        dtype = np.dtype(dtype)
        assert byte_offset % dtype.itemsize == 0
        if strides is None:
            strides, acc = [], 1
            for d in tuple(shape)[::-1]:
                strides.append(acc)
                acc *= d
            strides = strides[::-1]
        return DeviceArray(lib, arr.base_ptr, dtype, shape, strides, byte_offset // dtype.itemsize, arr._owner)

    def dev(host):
        return lib.to_device(np.ascontiguousarray(host))

    def rand(n, lo=1.0, hi=2.0):
        return rng.uniform(lo, hi, n).astype(f32)

    def bits(a):
        return np.ascontiguousarray(a).view(np.uint8).reshape(-1)

    def fill(arr, value):
        v = np.array([value], dtype=arr.dtype)
        lib._ck(lib.c.smhip_fill(C.c_int(sma.DTYPES[arr.dtype]), C.c_void_p(arr.ptr), v.ctypes.data_as(C.c_void_p), C.c_size_t(arr.size)))

    # ---- the ballast and the gates
    W = lib.to_device(np.ones(W_ELEMS, dtype=np.float64))
    ballast_call, _ = lib.chain_call(W, *[("pow", 1.37), ("pow", 0.73)] * (STAGES // 2), out=W)
    w_tail = W.ptr + W_ELEMS * 8 - GATE_MAX

    def gate_pattern(nbytes, dtype):
        return np.ones(nbytes // 8, dtype=np.float64).view(dtype)

    class Gate:
        def read(self, ptr, nbytes):       # the later writer of these bytes is behind the ballast (WAR)
            assert (512 << 10) <= nbytes <= GATE_MAX
            lib.copy(w_tail, ptr, nbytes)

        def write(self, ptr, nbytes):      # the later reader of these bytes is behind the ballast (RAW); they hold f64 ones
            assert (512 << 10) <= nbytes <= W_ELEMS * 8 - GATE_MAX and nbytes % 8 == 0
            lib.copy(ptr, W.ptr, nbytes)
    gate = Gate()

    results = []

    def race(name, issue, check, warm=None, ballast_queue=None):
        """warm(): every call of issue() once, outside the race.  issue(): gate, P, C.  check() -> None or what is wrong.
        ballast_queue: the queue the ballast must take (an operator that depends on nothing takes queue `alternations & 1`)."""
        if warm is not None:
            warm()
        ballast_call()
        lib.synchronize()
        if ballast_queue is not None and (lib.queue_stats()[1] & 1) != ballast_queue:  # one independent tracked operator more
            fill(flip_buf, 1.0)
            lib.synchronize()
        t0 = time.perf_counter()
        for _ in range(K_BALLAST):
            ballast_call()
        issue()
        t1 = time.perf_counter()
        lib.synchronize()
        t2 = time.perf_counter()
        detail = check()
        w = W.numpy()
        if not (w[: (W_ELEMS * 8 - GATE_MAX) // 8] == 1.0).all():
            detail = (detail or "") + " W's head is no longer all ones"
        lib.upload(w_tail, np.ones(GATE_MAX // 8, dtype=np.float64))
        lib.synchronize()
        rec = {"name": name, "ok": detail is None, "raced": (t2 - t1) >= (t1 - t0), "issue_ms": round(1e3 * (t1 - t0), 3), "drain_ms": round(1e3 * (t2 - t1), 3),
               "detail": detail}
        results.append(rec)
        print("RACE " + json.dumps(rec), flush=True)

    def same(what, got_dev, want):
        got = got_dev.numpy() if isinstance(got_dev, DeviceArray) else got_dev
        want = np.ascontiguousarray(want).reshape(got.shape) if want.size == got.size else want
        if got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want)):
            return None
        if got.shape != want.shape or got.dtype != want.dtype:
            return f"{what}: got {got.dtype}{got.shape}, want {want.dtype}{want.shape}"
        wrong = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        k = int(wrong[0]) if wrong.size else -1
        return f"{what}: {wrong.size} of {got.size} elements differ, first at {k}: got {got.reshape(-1)[k]!r}, want {want.reshape(-1)[k]!r}"

    def first(*details):
        for d in details:
            if d:
                return d
        return None

    flip_buf = lib.to_device(np.zeros(1 << 20, dtype=f32))
    if lib.queue_stats()[0] != 2:
        print(f"the device runs on {lib.queue_stats()[0]} queue(s), not 2: nothing here would race")
        return 2

    # ---------------------------------------------------------------------------------------------- the generic entry points
    # run(src, dst, aux): src, dst, aux dense 1-D f32 arrays of N elements; ref(src_h, aux_h, dst_before_h) -> dst_after_h
    oracle_obj = []

    def uniform_ref():
        if not oracle_obj:
            if not os.path.exists(orc.ORACLE_SO):
                orc.build(ref=False)
            oracle_obj.append(orc.Oracle())
        return oracle_obj[0].uniform_f32(N, 11, -1.0, 1.0)

    def v2(a, shape=(ROWS, COLS), strides=None):
        return view(a, f32, a.offset * 4, shape, strides)

    idx_h = rng.integers(0, N, N).astype(np.int64)
    idx_d = dev(idx_h)

    ENTRIES = {
        "copy": (True, lambda s, d, a: lib.copy(d.ptr, s.ptr, N * 4), lambda s, a, d0: s),
        "fill": (False, lambda s, d, a: fill(d, 3.25), lambda s, a, d0: np.full(N, 3.25, f32)),
        "fill_uniform": (False, lambda s, d, a: lib._ck(lib.c.smhip_fill_uniform_f32(C.c_void_p(d.ptr), N, 11, 0, -1.0, 1.0)), lambda s, a, d0: uniform_ref()),
        # the Generator's draw (smhip_random: a write span and nothing read), its bytes from the CPU model of tests/random_model.py
        "random": (False, lambda s, d, a: lib._ck(lib.random_raw(sma.RANDOM_UNIFORM, sma.F32, d.ptr, N, 29, 3, 5, (-2.0, 6.0))),
                   lambda s, a, d0: random_model.draw("uniform", f32, 29, 3, 5, N, (-2.0, 6.0))),
        "elementwise": (True, lambda s, d, a: lib.binary(sma.OP_ADD, v2(s), v2(a, (1, COLS)), out=v2(d)),
                        lambda s, a, d0: (s.reshape(ROWS, COLS) + a[:COLS].reshape(1, COLS)).reshape(-1)),
        "copy_strided": (True, lambda s, d, a: lib.assign(v2(d), v2(s, (ROWS, COLS), (1, ROWS))), lambda s, a, d0: s.reshape(COLS, ROWS).T.reshape(-1)),
        "contiguous": (True, lambda s, d, a: lib.contiguous(sma.OP_MUL, s, a, out=d), lambda s, a, d0: s * a),
        "array_scalar": (True, lambda s, d, a: lib.array_scalar(sma.OP_ADD, s, 1.5, out=d), lambda s, a, d0: s + f32(1.5)),
        "fused_contiguous": (True, lambda s, d, a: lib.fused(sma.OP_ADD, sma.OP_MUL, s, a, 0.5, out=d), lambda s, a, d0: (s + a) * f32(0.5)),
        "fused_expr": (True, lambda s, d, a: lib.fused_expr("a0 - a1", s, a, out=d), lambda s, a, d0: s - a),
        "fused_expr_bcast": (True, lambda s, d, a: lib.fused_expr_bcast("a0 - a1", v2(s), v2(a, (1, COLS)), out=v2(d)),
                             lambda s, a, d0: (s.reshape(ROWS, COLS) - a[:COLS].reshape(1, COLS)).reshape(-1)),
        "chain": (True, lambda s, d, a: lib.chain(s, ("sub", a), ("mul", 2.0), out=d), lambda s, a, d0: (s - a) * f32(2.0)),
        "unary": (True, lambda s, d, a: lib.unary("neg", s, out=d), lambda s, a, d0: -s),
        "convert": (True, lambda s, d, a: lib.astype(view(s, np.int32, s.offset * 4, (N,)), f32, out=d), lambda s, a, d0: s.view(np.int32).astype(f32)),
        "where": (True, lambda s, d, a: lib.where((a, "gt", 1.5), s, a, out=d), lambda s, a, d0: np.where(a > f32(1.5), s, a)),
        # barrier operators in both roles
        "reduce_axis": (True, lambda s, d, a: lib.reduce("max", v2(s), axis=0, out=view(d, f32, d.offset * 4, (COLS,))),
                        lambda s, a, d0: np.concatenate([s.reshape(ROWS, COLS).max(axis=0), d0[COLS:]])),
        "scan": (True, lambda s, d, a: lib.scan("cummax", v2(s), axis=1, out=d), lambda s, a, d0: np.maximum.accumulate(s.reshape(ROWS, COLS), axis=1).reshape(-1)),
        "take": (True, lambda s, d, a: lib.take(s, idx_d, mode="wrap", out=d), lambda s, a, d0: s[idx_h]),
        "where_dense_copy": (True, lambda s, d, a: lib.where((v2(a, (ROWS, COLS), (1, ROWS)), "gt", 1.5), v2(s), 0.0, out=v2(d)),
                             lambda s, a, d0: np.where(a.reshape(COLS, ROWS).T > f32(1.5), s.reshape(ROWS, COLS), f32(0)).reshape(-1)),
    }
    names = list(ENTRIES)
    readers = [n for n in names if ENTRIES[n][0]]

    def pairs(kind):
        """(P, C): every entry that can take a role of `kind` takes it at least once; partners rotate through the list."""
        can_p = readers if kind in ("war", "waw") else names
        can_c = readers if kind == "raw" else names
        out = []
        for i, p in enumerate(names):
            if p in can_p:
                out.append((p, next(names[(i + k) % len(names)] for k in range(1, len(names)) if names[(i + k) % len(names)] in can_c)))
        for j, c in enumerate(names):
            if c in can_c and all(c != q for _, q in out):
                out.append((next(names[(j - k) % len(names)] for k in range(1, len(names)) if names[(j - k) % len(names)] in can_p), c))
        return out

    def generic(kind):
        s_h, s2_h, a_h = rand(N), rand(N), rand(N)
        S, S2, A = dev(s_h), dev(s2_h), dev(a_h)
        X, R, Sp = lib.empty((N,), f32), lib.empty((N,), f32), lib.empty((N,), f32)
        wx, wr = lib.empty((N,), f32), lib.empty((N,), f32)
        g_h = gate_pattern(N * 4, f32)
        warmed = set()
        for p, c in pairs(kind):
            fp, fc = ENTRIES[p][1], ENTRIES[c][1]
            rp, rc = ENTRIES[p][2], ENTRIES[c][2]
            x0, r0 = np.full(N, 7.0, f32), np.full(N, -7.0, f32)
            lib.upload(X.ptr, x0)
            lib.upload(R.ptr, r0)

            def warm():
                for e in (p, c):
                    if e not in warmed:
                        ENTRIES[e][1](S, wx, A)
                        warmed.add(e)
                lib.copy(wr.ptr, wx.ptr, N * 4)
            if kind == "raw":
                def issue():
                    gate.read(X.ptr, N * 4)
                    fp(S, X, A)
                    fc(X, R, A)
                x1 = rp(s_h, a_h, x0)
                want = {"X": x1, "R": rc(x1, a_h, r0)}
            elif kind == "war":
                def issue():
                    gate.write(X.ptr, N * 4)
                    fp(X, R, A)
                    fc(S2, X, A)
                want = {"R": rp(g_h, a_h, r0), "X": rc(s2_h, a_h, g_h)}
            else:
                def issue():
                    gate.write(Sp.ptr, N * 4)
                    fp(Sp, X, A)
                    fc(S2, X, A)
                want = {"X": rc(s2_h, a_h, rp(g_h, a_h, x0))}
            race(f"{kind}: P {p}, C {c}", issue, lambda: first(*[same(k, {"X": X, "R": R}[k], v) for k, v in want.items()]), warm)

    # ---------------------------------------------------------------------------------------- where the declared span is tested
    MIB = 1 << 20

    def spans_a():
        # -- C's window overlaps X only in its last 256 KiB
        b0 = rand(N)
        s_h = rand(MIB // 2)
        B, S, R = dev(b0), dev(s_h), lib.empty((MIB // 2,), f32)
        px = view(B, f32, 4 * MIB, (MIB // 2,))            # P's 2 MiB: bytes [4 MiB, 6 MiB)
        cw = view(B, f32, 4 * MIB + 256 * 1024 - 2 * MIB, (MIB // 2,))   # C's 2 MiB window ends 256 KiB into it

        def reset():
            lib.upload(B.ptr, b0)
            lib.upload(R.ptr, np.full(MIB // 2, -7.0, f32))
        reset()

        def issue():
            gate.read(px.ptr, MIB)
            lib.array_scalar(sma.OP_ADD, S, 1.5, out=px)
            lib.unary("neg", cw, out=R)
        b1 = b0.copy()
        b1[MIB:MIB + MIB // 2] = s_h + f32(1.5)
        lo = (4 * MIB + 256 * 1024 - 2 * MIB) // 4
        race("span: RAW, the last 256 KiB of C's window", issue, lambda: first(same("B", B, b1), same("R", R, -b1[lo:lo + MIB // 2])), lambda: (issue(), reset()))
        reset()
        g1 = gate_pattern(MIB, f32)

        def issue():  # WAR: P reads the window (the gate wrote its last MiB), C overwrites [4 MiB, 6 MiB)
            gate.write(B.ptr + 4 * MIB + 256 * 1024 - MIB, MIB)
            lib.unary("neg", cw, out=R)
            lib.array_scalar(sma.OP_ADD, S, 1.5, out=px)
        old = b0.copy()
        g_lo = (4 * MIB + 256 * 1024 - MIB) // 4
        old[g_lo:g_lo + MIB // 4] = g1
        b2 = old.copy()
        b2[MIB:MIB + MIB // 2] = s_h + f32(1.5)
        race("span: WAR, the last 256 KiB of P's window", issue, lambda: first(same("R", R, -old[lo:lo + MIB // 2]), same("B", B, b2)), lambda: (issue(), reset()))

        # -- a stepped view whose last element is its only element inside X
        reset()
        nv, step, a0 = 262144, 4, 3
        last = a0 + step * (nv - 1)                       # element 1048575: the last one below byte 4 MiB
        sv = view(B, f32, a0 * 4, (nv,), (step,))
        xs = view(B, f32, last * 4, (MIB // 2,))           # X begins AT that element
        Rv = lib.empty((nv,), f32)

        def reset_v():
            reset()
            lib.upload(Rv.ptr, np.full(nv, -7.0, f32))
        reset_v()

        def issue():
            gate.read(xs.ptr, MIB)
            lib.assign(xs, S)
            lib.unary("neg", sv, out=Rv)
        b3 = b0.copy()
        b3[last:last + MIB // 2] = s_h
        race("span: RAW, a stepped view's last element", issue, lambda: first(same("B", B, b3), same("R", Rv, -b3[a0::step][:nv])), lambda: (issue(), reset_v()))
        reset_v()

        def issue():  # WAR: the gate writes the MiB that ends with the view's last element
            gate.write(B.ptr + 3 * MIB, MIB)
            lib.unary("neg", sv, out=Rv)
            lib.assign(xs, S)
        old = b0.copy()
        old[3 * MIB // 4:MIB] = g1
        b4 = old.copy()
        b4[last:last + MIB // 2] = s_h
        race("span: WAR, a stepped view's last element", issue, lambda: first(same("R", Rv, -old[a0::step][:nv]), same("B", B, b4)), lambda: (issue(), reset_v()))

        # -- a transposed view of X as an operand
        x0 = np.full(N, 7.0, f32)
        X, A, R2 = dev(x0), dev(rand(N)), lib.empty((N,), f32)
        s2 = rand(N)
        S2 = dev(s2)
        a_h = A.numpy()

        def reset_t():
            lib.upload(X.ptr, x0)
            lib.upload(R2.ptr, np.full(N, -7.0, f32))
        reset_t()

        def issue():
            gate.read(X.ptr, N * 4)
            lib.contiguous(sma.OP_MUL, S2, A, out=X)
            lib.binary(sma.OP_ADD, v2(X, (ROWS, COLS), (1, ROWS)), v2(A), out=v2(R2))
        x1 = s2 * a_h
        race("span: RAW, a transposed view", issue, lambda: first(same("X", X, x1), same("R", R2, (x1.reshape(COLS, ROWS).T + a_h.reshape(ROWS, COLS)).reshape(-1))),
             lambda: (issue(), reset_t()))

        # -- a stride-0 row inside X as the broadcast operand
        row_at = N // 2 + 3 * COLS
        for who in ("elementwise", "chain", "fused_expr_bcast"):
            reset_t()
            xr = view(X, f32, (N // 2) * 4, (MIB // 2,))         # P writes 2 MiB of X; the row lies inside
            row = view(X, f32, row_at * 4, (1, COLS), (0, 1))

            def issue():
                gate.read(xr.ptr, MIB)
                lib.array_scalar(sma.OP_MUL, S, 3.0, out=xr)
                if who == "elementwise":
                    lib.binary(sma.OP_MUL, v2(A), row, out=v2(R2))
                elif who == "chain":
                    lib.chain(v2(A), ("mul", row), ("add", 1.0), out=v2(R2))
                else:
                    lib.fused_expr_bcast("a0 * a1", v2(A), row, out=v2(R2))
            x2 = x0.copy()
            x2[N // 2:N // 2 + MIB // 2] = s_h * f32(3.0)
            want = a_h.reshape(ROWS, COLS) * x2[row_at:row_at + COLS].reshape(1, COLS)
            if who == "chain":
                want = want + f32(1.0)
            race(f"span: RAW, a stride-0 row as {who}'s operand", issue, lambda: first(same("X", X, x2), same("R", R2, want.reshape(-1))), lambda: (issue(), reset_t()))

    def spans_b():
        x0 = np.full(N, 7.0, f32)
        s_h, c_h, y_h, a_h = rand(N), rand(N), rand(N), rand(N)
        X, S, Cx, Cy, A, R = dev(x0), dev(s_h), dev(c_h), dev(y_h), dev(a_h), lib.empty((N,), f32)

        def reset():
            lib.upload(X.ptr, x0)
            lib.upload(R.ptr, np.full(N, -7.0, f32))
            lib.upload(A.ptr, a_h)
        # -- where with four array operands, only the last-named in X; then the same in place
        for in_place in (False, True):
            reset()
            out = A if in_place else R

            def issue():
                gate.read(X.ptr, N * 4)
                lib.array_scalar(sma.OP_ADD, S, 1.5, out=X)
                lib.where((Cx, "gt", Cy), A, X, out=out)
            x1 = s_h + f32(1.5)
            race("span: RAW, where's last operand" + (" in place" if in_place else ""), issue,
                 lambda: first(same("X", X, x1), same("out", out, np.where(c_h > y_h, a_h, x1))), lambda: (issue(), reset()))
        # -- a chain in place: P reads X (uploaded long ago) and G (which the gate writes: that keeps P behind the ballast); the chain
        # reads and overwrites X -- its one conflict is the WAR with P
        reset()
        g_h = gate_pattern(N * 4, f32)
        G = lib.empty((N,), f32)

        def issue():
            gate.write(G.ptr, N * 4)
            lib.contiguous(sma.OP_ADD, X, G, out=R)
            lib.chain(X, ("mul", A), ("sub", 0.25), out=X)
        race("span: WAR, a chain in place", issue, lambda: first(same("R", R, x0 + g_h), same("X", X, x0 * a_h - f32(0.25))), lambda: (issue(), reset()))
        # -- astype between element sizes, X as the source and as the destination
        n4 = MIB  # elements: f32 4 MiB -> f64 8 MiB; i64 8 MiB -> i32 4 MiB
        f_h = rand(n4)
        i_h = rng.integers(-2 ** 31, 2 ** 31, n4).astype(np.int64)
        F, I = dev(f_h), dev(i_h)
        X8, X4, R8, R4 = lib.empty((n4,), np.float64), lib.empty((n4,), f32), lib.empty((n4,), np.float64), lib.empty((n4,), f32)
        half8 = view(X8, np.float64, n4 * 4, (n4 // 2,))

        def reset_c():
            lib.upload(X8.ptr, np.full(n4, 7.0))
            lib.upload(X4.ptr, np.full(n4, 7.0, f32))
            lib.upload(R8.ptr, np.full(n4, -7.0))
            lib.upload(R4.ptr, np.full(n4, -7.0, f32))
        reset_c()

        def issue():
            gate.read(X4.ptr, n4 * 4)
            lib.array_scalar(sma.OP_ADD, F, 1.5, out=X4)
            lib.astype(X4, np.float64, out=R8)
        race("span: RAW, astype f32 -> f64 from X", issue, lambda: same("R", R8, (f_h + f32(1.5)).astype(np.float64)), lambda: (issue(), reset_c()))
        reset_c()
        r8h = view(R8, np.float64, 0, (n4 // 2,))

        def issue():  # the reader touches only the SECOND half of the f64 result: out_bytes must be n * 8
            gate.read(half8.ptr, n4 * 4)
            lib.astype(F, np.float64, out=X8)
            lib.unary("neg", half8, out=r8h)
        race("span: RAW, astype f32 -> f64 into X, its second half read", issue,
             lambda: first(same("X", X8, f_h.astype(np.float64)), same("R", R8, np.concatenate([-f_h[n4 // 2:].astype(np.float64), np.full(n4 // 2, -7.0)]))),
             lambda: (issue(), reset_c()))
        reset_c()
        X8i, half8i = view(X8, np.int64, 0, (n4,)), view(X8, np.int64, n4 * 4, (n4 // 2,))
        Ih = view(I, np.int64, 0, (n4 // 2,))
        R4i = view(R4, np.int32, 0, (n4,))
        lib.upload(X8.ptr, i_h[::-1].copy())

        def issue():  # the writer touches only the SECOND half of the i64 source: a_bytes must be n * 8
            gate.read(half8i.ptr, n4 * 4)
            lib.copy(half8i.ptr, Ih.ptr, n4 * 4)
            lib.astype(X8i, np.int32, out=R4i)
        xi = i_h[::-1].copy()
        xi[n4 // 2:] = i_h[:n4 // 2]

        def restore_i():
            reset_c()
            lib.upload(X8.ptr, i_h[::-1].copy())
        race("span: RAW, astype i64 -> i32 from X, its second half written", issue, lambda: same("R", R4i, xi.astype(np.int32)), lambda: (issue(), restore_i()))
        reset_c()
        X4i = view(X4, np.int32, 0, (n4,))

        def issue():
            gate.read(X4.ptr, n4 * 4)
            lib.astype(I, np.int32, out=X4i)
            lib.unary("neg", X4i, out=R4i)
        race("span: RAW, astype i64 -> i32 into X", issue, lambda: first(same("X", X4i, i_h.astype(np.int32)), same("R", R4i, -i_h.astype(np.int32))), lambda: (issue(), reset_c()))
        # -- one operator just under 1 MiB of operand bytes: a barrier operator, still right
        reset()
        small = 80000  # 3 x 320 000 bytes
        xs, As, Rs = view(X, f32, 0, (small,)), view(A, f32, 0, (small,)), view(R, f32, 0, (small,))
        xr = view(X, f32, 0, (MIB // 2,))
        Sh = view(S, f32, 0, (MIB // 2,))

        def issue():
            gate.read(xr.ptr, MIB)
            lib.array_scalar(sma.OP_ADD, Sh, 1.5, out=xr)
            lib.contiguous(sma.OP_ADD, xs, As, out=Rs)
        want = np.full(N, -7.0, f32)
        want[:small] = (s_h[:small] + f32(1.5)) + a_h[:small]
        race("span: RAW, an operator just under 1 MiB", issue, lambda: same("R", R, want), lambda: (issue(), reset()))

    def large():
        # one operator over 224 MiB of operand bytes: tracked, on queue 0 whatever it depends on -- so the ballast is put on queue 1,
        # or stream order alone would do
        nb = 64 << 20  # f32: 256 MiB
        b_h = rng.uniform(1.0, 2.0, nb).astype(f32)
        s_h = rand(MIB // 2)
        B, S, R = dev(b_h), dev(s_h), lib.empty((nb,), f32)
        xt = view(B, f32, (nb - MIB // 2) * 4, (MIB // 2,))
        b1 = b_h.copy()
        b1[-(MIB // 2):] = s_h * f32(3.0)
        want = b1 + f32(1.5)

        def reset():
            lib.upload(B.ptr, b_h)
            fill(R, -7.0)
        reset()

        def issue():
            gate.read(xt.ptr, MIB)
            lib.array_scalar(sma.OP_MUL, S, 3.0, out=xt)
            lib.array_scalar(sma.OP_ADD, B, 1.5, out=R)
        race("span: RAW, an operator over 224 MiB", issue, lambda: first(same("B tail", xt, b1[-(MIB // 2):]), same("R", R, want)), lambda: (issue(), reset()), ballast_queue=1)

    def tiny():
        x0 = np.full(N, 7.0, f32)
        s_h, a_h = rand(N), rand(N)
        X, S, A, R = dev(x0), dev(s_h), dev(a_h), lib.empty((N,), f32)
        t55 = view(X, f32, (N // 3) * 4, (5, 5), (COLS, 1))
        o_h = rand(25).reshape(5, 5)
        O = dev(o_h)

        def reset():
            lib.upload(X.ptr, x0)
            lib.upload(R.ptr, np.full(N, -7.0, f32))
        reset()
        got = {}

        def issue():  # a tiny operator reads 25 elements of X while P is still behind the ballast
            gate.read(X.ptr, N * 4)
            lib.array_scalar(sma.OP_ADD, S, 1.5, out=X)
            got["t"] = lib.binary(sma.OP_MUL, t55, O)
        x1 = s_h + f32(1.5)
        at = N // 3 + (np.arange(5) * COLS)[:, None] + np.arange(5)[None, :]
        race("tiny: RAW, 25 elements of X read by a recorded operator", issue, lambda: first(same("X", X, x1), same("t", got["t"], x1[at] * o_h)), lambda: (issue(), reset()))
        reset()

        def issue():  # a tiny operator is recorded reading a slice of X, then a large C overwrites X
            got["t"] = lib.binary(sma.OP_MUL, t55, O)
            lib.array_scalar(sma.OP_ADD, S, 1.5, out=X)
        race("tiny: WAR, a recorded operator's slice of X overwritten", issue, lambda: first(same("t", got["t"], x0[at] * o_h), same("X", X, x1)), lambda: (issue(), reset()), ballast_queue=0)
        reset()
        r_h = rand(COLS).reshape(1, COLS)
        Rw1, Rw2 = dev(r_h), dev(r_h + f32(1.0))

        def issue():  # a tiny result is the stride-0 operand of the large operator issued straight after it
            got["row"] = lib.binary(sma.OP_ADD, Rw1, Rw2)
            lib.binary(sma.OP_MUL, v2(A), got["row"], out=v2(R))
        row = r_h + (r_h + f32(1.0))
        race("tiny: RAW, a recorded result as a large operator's stride-0 operand", issue,
             lambda: first(same("row", got["row"], row), same("R", R, (a_h.reshape(ROWS, COLS) * row).reshape(-1))), lambda: (issue(), reset()), ballast_queue=0)

    def pool():
        s_h, a_h = rand(N), rand(N)
        S, A = dev(s_h), dev(a_h)
        Sp, R = lib.empty((N,), f32), lib.empty((N,), f32)
        g_h = gate_pattern(N * 4, f32)
        state = {}
        # -- WAW: P's result array is dropped before P has started; a new array takes its block and is filled by a tracked fill
        hits = 0
        for rep in range(3):
            state["T"] = lib.empty((N,), f32)
            state["old"] = state["T"].base_ptr

            def issue():
                gate.write(Sp.ptr, N * 4)
                lib.contiguous(sma.OP_MUL, Sp, A, out=state["T"])   # P: behind the ballast
                state["T"] = None                                    # dropped: back to the pool while P has not started
                state["new"] = lib.empty((N,), f32)
                fill(state["new"], 7.0)

            def warm():
                t = lib.empty((N,), f32)
                lib.contiguous(sma.OP_MUL, S, A, out=t)
                fill(t, 7.0)
            same_block = []

            def check():
                same_block.append(state["new"].base_ptr == state["old"])
                return same("the new array", state["new"], np.full(N, 7.0, f32))
            race(f"pool: WAW, a dropped result's block filled again (repetition {rep})", issue, check, warm)
            hits += bool(same_block and same_block[0])
            state["new"] = None
        rec = {"name": "pool: WAW reused the block", "ok": True, "raced": hits > 0, "detail": None if hits else "NOT EXERCISED: the new array never got the dropped one's address"}
        results.append(rec)
        print("RACE " + json.dumps(rec), flush=True)
        # -- WAR: P reads the dropped array
        hits = 0
        for rep in range(3):
            state["D"] = lib.empty((N,), f32)
            state["old"] = state["D"].base_ptr
            lib.upload(R.ptr, np.full(N, -7.0, f32))

            def issue():
                gate.write(state["D"].ptr, N * 4)
                lib.contiguous(sma.OP_MUL, state["D"], A, out=R)    # P reads D, behind the ballast
                state["D"] = None
                state["new"] = lib.empty((N,), f32)
                fill(state["new"], 7.0)
            same_block = []

            def check():
                same_block.append(state["new"].base_ptr == state["old"])
                return first(same("R", R, g_h * a_h), same("the new array", state["new"], np.full(N, 7.0, f32)))
            race(f"pool: WAR, a dropped operand's block filled again (repetition {rep})", issue, check, warm)
            hits += bool(same_block and same_block[0])
            state["new"] = None
        rec = {"name": "pool: WAR reused the block", "ok": True, "raced": hits > 0, "detail": None if hits else "NOT EXERCISED: the new array never got the dropped one's address"}
        results.append(rec)
        print("RACE " + json.dumps(rec), flush=True)
        # -- WAR through an operator's own scratch, and the chain whose result is cut through pooled temporaries: three P read three
        # arrays (uploaded long ago; their other operand G is what the gate writes, which keeps them behind the ballast) that are
        # dropped at once; two cut chains (f64 exp / log stages) then take their temporaries from the pool
        n64 = N // 2
        d_h = rng.uniform(1.0, 2.0, n64)
        Z, D64 = dev(np.zeros(n64)), dev(d_h)
        R64 = [lib.empty((n64,), np.float64) for _ in range(2)]
        R2 = [lib.empty((n64,), np.float64) for _ in range(3)]
        cut = (("exp",), ("add", D64), ("log",), ("exp",), ("mul", 2.0))  # exp(0) = 1 exactly; the rest is checked against a run alone
        for r in R2:
            lib.upload(r.ptr, np.full(n64, -7.0))
        G64 = lib.empty((n64,), np.float64)
        dk_h = [rng.uniform(1.0, 2.0, n64) for _ in range(3)]
        state["D"] = [dev(h) for h in dk_h]

        def issue():
            gate.write(G64.ptr, n64 * 8)
            for k in range(3):
                lib.contiguous(sma.OP_ADD, state["D"][k], G64, out=R2[k])  # P reads D[k] and G (f64 ones), behind the ballast
            state["D"] = None                                                # all three back to the pool
            for r in R64:
                lib.chain(Z, *cut, out=r)                                    # C: its temporaries come from the pool

        def warm64():
            t = lib.empty((n64,), np.float64)
            lib.contiguous(sma.OP_ADD, Z, D64, out=t)
            lib.chain(Z, *cut, out=R64[0])

        def check():
            alone = lib.chain(Z, *cut).numpy()
            near = np.allclose(alone, (1.0 + d_h) * 2.0, rtol=1e-12, atol=0)
            return first(*[same(f"R{k}", R2[k], dk_h[k] + 1.0) for k in range(3)], None if near else "the chain's own value is not 2 (1 + d)",
                         *[same(f"chain {k} (against the chain run alone)", r, alone) for k, r in enumerate(R64)])
        race("pool: WAR, dropped operands' blocks as the temporaries of cut chains", issue, check, warm64)

    {"raw": lambda: generic("raw"), "war": lambda: generic("war"), "waw": lambda: generic("waw"), "spans_a": spans_a, "spans_b": spans_b, "large": large,
     "tiny": tiny, "pool": pool}[group]()
    lib.synchronize()
    bad = [r for r in results if not (r["ok"] and r["raced"])]
    print("RACE " + json.dumps({"done": group, "scenarios": len(results), "failed": len(bad), "queues": lib.queue_stats()}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1]))
