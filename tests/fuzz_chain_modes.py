"""Second soak for smhip_chain / smhip_chain_sum (csrc/chain.hip), beside tests/fuzz_chain.py (whose cases it leaves as they are):
random chains of 1 to 12 stages over every STAGE KIND -- + - * / over fuzz_chain's operand forms, ^s (s = 2 fused, s = 1 dropped, any
other exponent a cut), neg / abs / sqrt / exp / log -- written in every OUTPUT MODE: a fresh array, a preallocated one, IN PLACE
(out is a dense operand of the chain, possibly several of them), and a dense block of rows of a taller array; one case in four is
also SUMMED (smhip_chain_sum) from the original operands.

Reference, stage by stage on the host in the element type: + - * / and ^2 (one product) by the oracle, ^1 / neg / abs / sqrt by
numpy -- exact; exp, log and every other exponent by the STANDALONE GPU operator (lib.unary, lib.array_scalar(OP_POW)) applied to
the uploaded reference value so far -- the chain's contract is "the same bits as the operators called one by one" -- and that
standalone result is itself held to the operator's own bar against a wider evaluation (1 ULP for exp / log as in
tests/test_unary_gpu.py; pow: 4 ULP of the correctly rounded value for f32, 1 ULP of libm's pow for f64, as in
tests/test_gpu_parity.py; integer powers exactly, wrapping).  The chain's output is compared bit for bit, NaN to NaN.
An integer stage that would divide by zero or INT_MIN by -1 is drawn again before it is committed: no case is skipped.

    usage: python tests/fuzz_chain_modes.py [cases] [seed] [trace] [--plan-only]
--plan-only draws the cases and prints the coverage table without loading a device (exp / log / general powers of floats are then
numpy's: good enough to count the cases whose reference holds a NaN or an infinity)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplemath_amd as sma
from oracle import oracle as orc
from tests import util
from tests.fuzz_chain import values, random_shape, operand

DT = [np.float32, np.float32, np.float64, np.int32, np.int64]
OPS = [sma.OP_ADD, sma.OP_SUB, sma.OP_MUL, sma.OP_DIV]
ORC = {sma.OP_ADD: orc.ADD, sma.OP_SUB: orc.SUB, sma.OP_MUL: orc.MUL, sma.OP_DIV: orc.DIV}
MAX_ELEMENTS = 1 << 17
MAX_STAGES = 12
POW_F = [2, 1, 3, 0.5, 2.5, -1]
POW_I = [2, 1, 3, 0]
POW_ULP_F32 = 4  # tests/test_gpu_parity.py: POW_ULP, of the correctly rounded value
POW_ULP_F64 = 1  # ... and of libm's pow for f64
MODES = ["fresh", "preallocated", "in place", "row block"]
ALONE = ["transposed operand", "stepped operand", "log", "f64 exp", "general pow"]
ROWS = ([f"stage {k}" for k in ("+-*/", "^2", "^1", "^other", "neg", "abs", "sqrt", "exp f32 (fused)", "exp f64 (cut)", "log")]
        + ["stage +-*/ with a view operand (cut)", "five or more distinct dense operands", "two or more distinct rows"]
        + [f"out: {m}" for m in MODES]
        + [f"in place, last stage alone: {k}" for k in ALONE]
        + ["in place, read after a cutting stage", "in place, read behind a fifth dense operand", "in place, one array as several operands",
           "row block that is also an operand", "view head directly under a function or a power", "broadcast head directly under a function",
           "broadcast head directly under a power", "written-out periodic head directly under log / f64 exp", "sum mode"])


class Redraw(Exception):
    """the stage just drawn would trap in the reference (integer division by zero, INT_MIN / -1)"""


class BarMiss(Exception):
    """a standalone operator missed its own bar: the reference of this soak is not to be trusted"""


def shape_up_to(rng, limit):
    while True:
        shape = random_shape(rng)
        if int(np.prod(shape)) <= limit:
            return shape


def view_operand(rng, shape, dt, kind):
    """a transposed / stepped operand as fuzz_chain.operand builds them -> (host view, (base, view), label)"""
    if kind == "T" and len(shape) >= 2:
        base = values(rng, shape[::-1], dt)
        return base.T, (base, base.T), "T"
    wide = list(shape); wide[-1] = shape[-1] * 2 + 1
    base = values(rng, tuple(wide), dt)
    view = base[..., ::2][..., :shape[-1]]
    return view, (base, view), "step"


def is_view(h):
    return isinstance(h, np.ndarray) and not h.flags.c_contiguous


def int_division_traps(dividend, divisor):
    dividend, divisor = np.broadcast_arrays(np.asarray(dividend), np.asarray(divisor))
    if (divisor == 0).any():
        return True
    return bool(((dividend == np.iinfo(dividend.dtype).min) & (divisor == -1)).any())


class Reference:
    """One stage at a time on the host; `lib` None: no device, inexact float stages by numpy (planning only)."""

    def __init__(self, o, lib):
        self.o, self.lib = o, lib
        self.ulp = None
        if lib is not None:
            from tests.test_unary_gpu import ulp_distance, true_value  # the 1 ULP bar of exp / log, as that suite measures it
            self.ulp, self.true_value = ulp_distance, true_value

    def standalone(self, what, r, call, want_of):
        """the standalone GPU operator on the uploaded value so far, held to its own bar"""
        x = np.ascontiguousarray(r)
        d = self.lib.to_device(x)
        res = call(d)
        got = res.numpy().reshape(x.shape)
        worst, bar = want_of(x, got)
        if not worst <= bar:
            raise BarMiss(f"standalone {what} ({x.dtype.name}, {x.shape}): {worst} ULP from the wide evaluation, bar {bar}")
        return got

    def apply(self, r, st):
        o, dt = self.o, r.dtype
        kind = st["kind"]
        if kind == "op":
            op, h, swapped = st["op"], st["h"], st["swapped"]
            if dt.kind == "i" and op == sma.OP_DIV and (int_division_traps(h, r) if swapped else int_division_traps(r, h)):
                raise Redraw
            if isinstance(h, np.ndarray):
                return o.binary(ORC[op], h, r) if swapped else o.binary(ORC[op], r, h)
            return o.array_scalar(ORC[op], np.ascontiguousarray(r).reshape(-1), h).reshape(r.shape)
        if kind == "pow":
            e = st["e"]
            if e == 2:
                return o.binary(orc.MUL, r, r)
            if e == 1:
                return r
            with np.errstate(all="ignore"):
                if dt.kind == "i":  # exact, wrapping: x^3 = x*x*x, x^0 = 1 (0^0 included)
                    exact = np.power(r, dt.type(e))
                    if self.lib is None:
                        return exact
                    return self.standalone(f"^{e}", r, lambda d: self.lib.array_scalar(sma.OP_POW, d, dt.type(e)),
                                           lambda x, got: (0 if np.array_equal(got, exact) else np.inf, 0))
                if self.lib is None:
                    return np.power(r, dt.type(e))
                if dt == np.float32:
                    bar = lambda x, got: (int(orc.ulp_diff_f32(got, np.power(x.astype(np.float64), e).astype(np.float32)).max()), POW_ULP_F32)
                else:
                    bar = lambda x, got: (int(orc.ulp_diff_f64(got, o.array_scalar(orc.POW, x.reshape(-1), e).reshape(x.shape)).max()), POW_ULP_F64)
                return self.standalone(f"^{e}", r, lambda d: self.lib.array_scalar(sma.OP_POW, d, dt.type(e)), bar)
        fn = st["fn"]
        with np.errstate(all="ignore"):
            if fn == "neg":
                return np.negative(r)
            if fn == "abs":
                return np.abs(r)
            if fn == "sqrt":
                return np.sqrt(r)
            if self.lib is None:
                return {"exp": np.exp, "log": np.log}[fn](r)
            return self.standalone(fn, r, lambda d: self.lib.unary(fn, d),
                                   lambda x, got: (float(self.ulp(got, self.true_value(fn, x)).max()), 1.0))


def draw_case(rng, ref):
    """-> a dict: everything about the case, host side; integer stages are evaluated (exactly) as they are drawn"""
    dt = DT[int(rng.integers(0, len(DT)))]
    isf = np.dtype(dt).kind == "f"
    shape = shape_up_to(rng, MAX_ELEMENTS)
    nd = len(shape)
    mode = MODES[int(rng.choice(4, p=[0.2, 0.15, 0.45, 0.2]))]
    force = [None, "dense", "row"][int(rng.choice(3, p=[0.55, 0.3, 0.15]))]
    summed = bool(rng.random() < 0.25)
    tail = None
    if mode == "in place" and rng.random() < 0.7:
        kinds = ["T", "step", "pow"] + (["log"] if isf else []) + (["exp"] * 5 if dt == np.float64 else [])
        tail = kinds[int(rng.integers(0, len(kinds)))]
    under = bool(rng.random() < 0.3)
    periodic_head = under and bool(rng.random() < 0.5)
    if periodic_head:  # the reference tests' (1,d1,1,d3) in (d0,d1,d2,d3): classify() has the period written out when it repeats four times or more
        shape = tuple(int(rng.choice(c)) for c in ([4, 5, 7, 8], [2, 3, 5, 7, 12], [2, 3, 4, 5, 8], [2, 3, 4, 5, 7, 16]))
        nd = 4
    # the in-place operand: a dense array of the full shape, or (row block) the block itself
    X = tall = block = None
    if mode == "in place":
        X = values(rng, shape, dt)
        xspec = X
    elif mode == "row block" and rng.random() < 0.5:
        tall, block = make_tall(rng, shape, dt)
        X, xspec = block, (tall, block)
    n_rand = int(rng.integers(1, MAX_STAGES + 1))
    head_dense = bool(rng.random() < 0.5)
    forced = []
    if force == "dense":
        forced = ["dense"] * (4 if head_dense else 5)
    elif force == "row":
        forced = ["row"] * 2
    tail_len = 0 if tail is None else 2 if tail in ("log", "pow") else 1
    # a head that is not dense with a function or a power DIRECTLY on it: nothing to apply it to in place (chain.hip: head_plain,
    # head_view), and a periodic head's written-out copy must not stand in for it where the stage runs alone (original_of)
    tail_len += 1 if under else 0
    n_rand = max(0 if forced or tail else 1, min(n_rand, MAX_STAGES - len(forced) - tail_len))
    script = ["rand"] * n_rand + forced
    for _ in range(len(forced)):  # the forced operands among the others, not always at the end
        i, j = int(rng.integers(0, len(script))), int(rng.integers(0, len(script)))
        script[i], script[j] = script[j], script[i]
    # where the chain reads X
    x_head, x_at = False, set()
    if X is not None:
        where = ["head", "middle", "last"][int(rng.integers(0, 3))]
        if not script or where == "head":
            x_head = True
        elif where == "last" and tail in (None, "log", "exp", "pow"):
            x_at.add(len(script) - 1)
        else:
            x_at.add(int(rng.integers(0, len(script))))
        if rng.random() < 0.3:  # the same array as several operands
            x_head = x_head or bool(rng.random() < 0.5)
            if script:
                x_at.add(int(rng.integers(0, len(script))))
    for k in x_at:
        script[k] = "X"
    if tail in ("T", "step"):
        script.append(tail)
    elif tail == "log":
        script += ["abs" if rng.random() < 0.5 else "neg", "log"]
    elif tail == "exp":
        script.append("exp")
    elif tail == "pow":
        script += (["abs"] if isf and rng.random() < 0.5 else []) + [("pow", 2.5 if isf else 3)]
    under = under and not x_head
    periodic_head = periodic_head and under
    if periodic_head:
        firsts = ["log", "log", "log", "exp", ("pow", 2.5), "abs"] if isf else [("pow", 3), ("pow", 0), "neg"]
        script.insert(0, firsts[int(rng.integers(0, len(firsts)))])
    elif under:
        firsts = ["neg", "abs", ("pow", 2), ("pow", 3)] + (["sqrt", "exp", "exp", "log", "log", ("pow", 2.5)] if isf else [("pow", 0), ("pow", 1)])
        script.insert(0, firsts[int(rng.integers(0, len(firsts)))])
    # the head
    if x_head:
        head_h, head_d, label = X, xspec, "X"
    elif periodic_head:
        head_h = values(rng, (1, shape[1], 1, shape[3]), dt)
        head_d, label = head_h, "periodic"
    elif under:
        head_h, head_d, label = operand(rng, shape, dt)
        while label not in ("row", "col", "mid", "periodic", "T", "step", "pitch"):
            head_h, head_d, label = operand(rng, shape, dt)
    elif head_dense:
        head_h = values(rng, shape, dt)
        head_d, label = head_h, "dense"
    else:
        head_h, head_d, label = operand(rng, shape, dt)
        while not isinstance(head_h, np.ndarray):
            head_h, head_d, label = operand(rng, shape, dt)
    stages, labels = [], [label]
    r = np.ascontiguousarray(head_h)

    def commit(st, label):
        nonlocal r
        r = ref.apply(r, st)  # Redraw leaves everything as it was
        stages.append(st)
        labels.append(label)

    def op_stage(h, d, label):
        for _ in range(64):
            op = int(rng.choice(OPS))
            swapped = bool(rng.random() < 0.3) and isinstance(h, np.ndarray)
            try:
                commit({"kind": "op", "op": op, "h": h, "d": d, "swapped": swapped, "form": label}, ("~" if swapped else "") + "+-*/"[op] + label)
                return
            except Redraw:
                continue
        raise AssertionError("no operator could be drawn for this operand in 64 tries")

    room = MAX_STAGES - len(script)
    for what in script:
        if what == "rand":
            what = ["op", "op", "op", "op", "op", "op", "pow", "pow", "un", "un"][int(rng.integers(0, 10))]
            if what == "un":
                fns = ["neg", "abs"] + (["sqrt", "exp", "log"] if isf else [])
                what = fns[int(rng.integers(0, len(fns)))]
            elif what == "pow":
                es = POW_F if isf else POW_I
                what = ("pow", es[int(rng.integers(0, len(es)))])
            # both domains of sqrt, log and the non-integer powers, and their NaN path: an abs stage first, every other time
            if (what in ("sqrt", "log") or what in (("pow", 0.5), ("pow", 2.5))) and rng.random() < 0.5 and room > 0:
                room -= 1
                commit({"kind": "un", "fn": "abs"}, "abs")
        if what == "op":
            for _ in range(64):
                h, d, label = operand(rng, shape, dt)
                op = int(rng.choice(OPS))
                swapped = bool(rng.random() < 0.3) and isinstance(h, np.ndarray)
                try:
                    commit({"kind": "op", "op": op, "h": h, "d": d, "swapped": swapped, "form": label}, ("~" if swapped else "") + "+-*/"[op] + label)
                    break
                except Redraw:
                    continue
            else:
                raise AssertionError("no operator stage could be drawn in 64 tries")
        elif what == "X":
            op_stage(X, xspec, "X")
        elif what == "dense":
            h = values(rng, shape, dt)
            op_stage(h, h, "dense")
        elif what == "row":
            h = values(rng, (1,) * (nd - 1) + (shape[-1],), dt)
            op_stage(h, h, "row")
        elif what in ("T", "step"):
            h, d, label = view_operand(rng, shape, dt, what)
            op_stage(h, d, label)
        elif isinstance(what, tuple):
            commit({"kind": "pow", "e": what[1]}, f"^{what[1]}")
        else:
            commit({"kind": "un", "fn": what}, what)
    rshape = tuple(r.shape)
    if mode == "row block" and tall is None:
        tall, block = make_tall(rng, rshape, dt)
    case = dict(dt=dt, shape=shape, rshape=rshape, mode=mode, head_h=head_h, head_d=head_d, stages=stages, labels=labels, summed=summed,
                X=X, tall=tall, block=block, want=np.ascontiguousarray(r))
    case["stale"] = values(rng, rshape, dt) if mode == "preallocated" else None
    case["tags"] = tags_of(case)
    return case


def make_tall(rng, shape, dt):
    above, below = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    if above + below == 0:
        below = 1
    tall = values(rng, (above + shape[0] + below,) + tuple(shape[1:]), dt)
    return tall, tall[above:above + shape[0]]


def tags_of(case):
    dt, stages, X, mode, rshape = case["dt"], case["stages"], case["X"], case["mode"], case["rshape"]
    tags = {f"out: {mode}"}
    if case["summed"]:
        tags.add("sum mode")
    is_x = lambda h: X is not None and h is X
    dense = lambda h: isinstance(h, np.ndarray) and h.flags.c_contiguous and tuple(h.shape) == rshape
    seen_dense, seen_rows, cut_before = [], [], False
    reads = int(is_x(case["head_h"]))
    if dense(case["head_h"]):
        seen_dense.append(id(case["head_h"]))
    head = case["head_h"]
    if stages[0]["kind"] != "op" and not dense(head):
        first = stages[0]
        cutting = (first["kind"] == "pow" and first["e"] not in (1, 2)) or (first["kind"] == "un" and (first["fn"] == "log" or (first["fn"] == "exp" and dt == np.float64)))
        if is_view(head):
            tags.add("view head directly under a function or a power")
        elif first["kind"] == "pow":
            tags.add("broadcast head directly under a power")
        else:
            tags.add("broadcast head directly under a function")
        if first["kind"] == "un" and cutting and head.ndim == 4 and len(rshape) == 4 and head.shape[0] == head.shape[2] == 1 and min(head.shape[1], head.shape[3]) > 1 \
                and rshape[0] >= 4 and rshape[2] > 1:
            tags.add("written-out periodic head directly under log / f64 exp")
    for k, st in enumerate(stages):
        last = k == len(stages) - 1
        cuts = alone = None
        if st["kind"] == "op":
            tags.add("stage +-*/")
            h = st["h"]
            if is_view(h) and st["form"] in ("T", "step"):
                cuts = alone = {"T": "transposed operand", "step": "stepped operand"}[st["form"]]
                tags.add("stage +-*/ with a view operand (cut)")
            elif is_view(h):
                cuts = "pitched operand"
            if dense(h) and id(h) not in seen_dense:
                seen_dense.append(id(h))
            if isinstance(h, np.ndarray) and not dense(h) and h.flags.c_contiguous and h.ndim == len(rshape) and h.shape[-1] == rshape[-1] > 1 \
                    and h.size < int(np.prod(rshape)) and all(id(h) != q for q in seen_rows):
                seen_rows.append(id(h))
            if is_x(h):
                reads += 1
                if mode == "in place" and cut_before:
                    tags.add("in place, read after a cutting stage")
                if mode == "in place" and len(seen_dense) >= 5:
                    tags.add("in place, read behind a fifth dense operand")
        elif st["kind"] == "pow":
            e = st["e"]
            tags.add("stage ^2" if e == 2 else "stage ^1" if e == 1 else "stage ^other")
            if e not in (1, 2):
                cuts = alone = "general pow"
        else:
            fn = st["fn"]
            if fn == "exp":
                tags.add("stage exp f32 (fused)" if dt == np.float32 else "stage exp f64 (cut)")
                if dt == np.float64:
                    cuts = alone = "f64 exp"
            else:
                tags.add(f"stage {fn}")
                if fn == "log":
                    cuts = alone = "log"
        if last and alone and mode == "in place":
            tags.add(f"in place, last stage alone: {alone}")
        cut_before = cut_before or cuts is not None
    if len(seen_dense) >= 5:
        tags.add("five or more distinct dense operands")
    if len(seen_rows) >= 2:
        tags.add("two or more distinct rows")
    if mode == "in place" and reads >= 2:
        tags.add("in place, one array as several operands")
    if mode == "row block" and X is not None:
        tags.add("row block that is also an operand")
    return tags


def has_nonfinite(want):
    return want.dtype.kind == "f" and not np.isfinite(want).all()


def exact_sum(want):
    """-> (the exact sum as a float, sum of magnitudes)"""
    flat = want.reshape(-1)
    if want.dtype.kind == "f":
        return math.fsum(flat.tolist()), math.fsum(np.abs(flat).tolist())
    total = sum(flat.tolist()) % (1 << 64)
    if total >= 1 << 63:
        total -= 1 << 64
    return float(total), float(sum(abs(v) for v in flat.tolist()))


def describe(case):
    dn = np.dtype(case["dt"]).name
    return f"{dn} {case['shape']} -> {case['rshape']} [{case['mode']}{', summed' if case['summed'] else ''}] {' '.join(case['labels'])}"


def run_case(lib, ref, case, idx, seed, trace, stats):
    """-> True when the chain (and its sum) matched; the reference is evaluated again here, inexact stages on the device"""
    dt, mode = case["dt"], case["mode"]
    r = np.ascontiguousarray(case["head_h"])
    for st in case["stages"]:
        r = ref.apply(r, st)
    want = np.ascontiguousarray(r)
    bases = {}

    def to_dev(x):
        if isinstance(x, tuple):
            base, view = x
            if id(base) not in bases:
                bases[id(base)] = lib.to_device(base)
            return bases[id(base)].view_like(view, base)
        if isinstance(x, np.ndarray):
            if id(x) not in bases:
                bases[id(x)] = lib.to_device(x)
            return bases[id(x)]
        return x

    dhead = to_dev(case["head_d"])
    dstages = []
    for st in case["stages"]:
        if st["kind"] == "op":
            dstages.append((st["op"], to_dev(st["d"]), st["swapped"]))
        elif st["kind"] == "pow":
            dstages.append((sma.OP_POW, dt(st["e"])))
        else:
            dstages.append((st["fn"],))
    out = dtall = None
    if mode == "preallocated":
        out = lib.to_device(case["stale"])
    elif mode == "in place":
        out = to_dev(case["X"])
    elif mode == "row block":
        if id(case["tall"]) not in bases:
            bases[id(case["tall"])] = lib.to_device(case["tall"])
        dtall = bases[id(case["tall"])]
        out = dtall.view_like(case["block"], case["tall"])
    if trace:  # which case was in flight when something went wrong on the GPU
        def sh(x):
            return (tuple(x.shape), tuple(x.strides), x.offset) if isinstance(x, sma.DeviceArray) else x
        trace.write(f"case {idx}: {describe(case)} :: head {sh(dhead)} " + " ".join(f"[{st[0]} {sh(st[1]) if len(st) > 1 else ''}{' ~' if len(st) > 2 and st[2] else ''}]" for st in dstages)
                    + f" out {sh(out) if out is not None else 'fresh'}\n")
        trace.flush()
        os.fsync(trace.fileno())
    try:
        total = None
        if case["summed"]:  # from the original operands: before an in-place run overwrites one
            total = lib.chain_sum(dhead, *dstages)
        got = lib.chain(dhead, *dstages, out=out)
        if trace:
            lib.synchronize()
    except Exception as e:  # noqa: BLE001
        print(f"case {idx}: {describe(case)}: {e}")
        raise
    if mode == "row block":
        whole = dtall.numpy()
        lo = (case["block"].__array_interface__["data"][0] - case["tall"].__array_interface__["data"][0]) // case["tall"][0:1].nbytes
        g = whole[lo:lo + want.shape[0]]
        outside = np.ones(whole.shape[0], dtype=bool)
        outside[lo:lo + want.shape[0]] = False
        if whole[outside].tobytes() != case["tall"][outside].tobytes():
            print(f"MISMATCH case {idx} seed {seed}: {describe(case)}: rows outside the block were written")
            return False
    else:
        g = got.numpy()
    ok = g.shape == want.shape and g.dtype == want.dtype and bool(util.same_bits(g, want).all())  # NaN payloads are not part of the bar
    if not ok:
        bad = np.flatnonzero(~util.same_bits(g, want).reshape(-1)) if g.shape == want.shape else np.arange(0)
        print(f"MISMATCH case {idx} seed {seed}: {describe(case)}: {bad.size} of {g.size} elements, first at {bad[:5]}: "
              f"{g.reshape(-1)[bad[:3]] if bad.size else g.shape} want {want.reshape(-1)[bad[:3]] if bad.size else want.shape}")
        return False
    if case["summed"]:
        if has_nonfinite(want):
            stats["sum_nonfinite"] += 1
        else:
            s, scale = exact_sum(want)
            if np.dtype(dt).kind == "f":
                fine = abs(total - s) <= 1e-15 * scale + 1e-300
            else:
                fine = total == s
            if not fine:
                print(f"MISMATCH case {idx} seed {seed}: {describe(case)}: chain_sum {total!r} want {s!r} (sum of magnitudes {scale!r})")
                return False
            stats["sum_checked"] += 1
    return True


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    plan_only = "--plan-only" in sys.argv[1:]
    cases = int(argv[0]) if len(argv) > 0 else 300
    seed = int(argv[1]) if len(argv) > 1 else 1
    rng = np.random.default_rng(seed)
    o = orc.Oracle()
    lib = None if plan_only else sma.load()
    planner = Reference(o, None)
    ref = planner if plan_only else Reference(o, lib)
    trace = open(argv[2], "w") if len(argv) > 2 and not plan_only else None
    counts = {row: 0 for row in ROWS}
    stats = {"sum_checked": 0, "sum_nonfinite": 0}
    done = 0
    for idx in range(cases):
        case = draw_case(rng, planner)  # the draw never looks at the device: --plan-only sees the cases a run gets
        for t in case["tags"]:
            counts[t] += 1
        if plan_only:
            if case["summed"]:
                stats["sum_nonfinite" if has_nonfinite(case["want"]) else "sum_checked"] += 1
        elif not run_case(lib, ref, case, idx, seed, trace, stats):
            return 1
        done += 1
    print("coverage (cases that contain each):")
    for row in ROWS:
        print(f"  {counts[row]:5d}  {row}")
    print(f"sum mode: {stats['sum_checked']} compared, {stats['sum_nonfinite']} with a NaN or an infinity in the reference (not compared)")
    print(f"{'planned' if plan_only else 'ok'}: {done} chains, seed {seed}, skipped {cases - done}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
