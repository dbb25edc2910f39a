"""Small models for the tests of the tape sweep (tests/test_tape_sweep_cpu.py, tests/test_tape_sweep_gpu.py), all built
through model.Model / model.NlpProblem so that the oracle, the product and the mpmath reference (mpref.py) get the same
graph.

ops_model    every opcode at many points: a variable pair, three or four rows and the batch dimension as the points
chain_model  every differentiable op in ONE connected component, sized by L into the task class wanted
mixed_model  a 12-stage family, a large (256-thread) component and, optionally, a global-memory component in one problem

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import math

import numpy as np

from . import model

# ---- chain_model -----------------------------------------------------------------------------------------------------
# The order puts ops outside the basic set (tape_ops.h: op_is_basic) first: a chain of L = 4 steps, the stage of the
# 12-stage family, applies the first eight.
CHAIN_OPS = ["POW", "ATAN2", "EXP", "HYPOT", "LOG", "TANH", "ERF", "CBRT", "TAN", "ASIN", "SINH", "ACOS", "COSH", "ATAN",
             "LOG10", "SQRT", "DIV", "MAX", "MUL", "MIN", "ABS", "SIN", "COS", "SUB", "ADD", "NEG"]
BINARY = {"ADD", "SUB", "MUL", "DIV", "POW", "ATAN2", "HYPOT", "MAX", "MIN"}

# Where an op's domain is not the whole line its argument is centre + halfwidth * sin(t): inside the domain with margin
# whatever the chain's state t is.  (left, right) for a binary op; None: t as it is.
POSITIVE = (1.5, 0.9)
CHAIN_ARGS = {
    "POW": (POSITIVE, (0.5, 1.0)), "ATAN2": (POSITIVE, None), "HYPOT": (POSITIVE, None), "DIV": (None, POSITIVE),
    "EXP": ((0.0, 1.0),), "LOG": (POSITIVE,), "LOG10": (POSITIVE,), "SQRT": (POSITIVE,), "CBRT": (POSITIVE,),
    "TAN": ((0.0, 1.0),), "ASIN": ((0.0, 0.7),), "ACOS": ((0.0, 0.7),), "SINH": ((0.0, 1.5),), "COSH": ((0.3, 1.2),),
}
CHAIN_CONSTANTS = (0.6, 0.4, 0.25, 0.3)  # the four that chain_model can turn into parameters


class TapeModel:
    """p: model.NlpProblem; x: decision variables; x0: a start inside every op's domain; params: parameter variables."""

    def __init__(self, p, x, x0, params=()):
        self.p, self.x, self.x0, self.params = p, x, np.asarray(x0, dtype=np.float64), list(params)

    @property
    def dims(self):
        return self.p.p.dims

    @property
    def param_ids(self):
        return [v.node for v in self.params]

    def close(self):
        self.p.p.close()


def _apply(m, op, t, t2):
    def arg(spec, value):
        return value if spec is None else spec[0] + spec[1] * m.sin(value)

    spec = CHAIN_ARGS.get(op, (None, None))
    l = arg(spec[0], t)
    if op in BINARY:
        r = arg(spec[1], t2)
        return m._bi(op, l, r)
    return m._un(op, l)


def _component(m, p, n, L, start, consts, first_op=0):
    """One connected component on n new decision variables: L non-contracting residual updates
         a <- a + step * phi_k (w_b * b + w_x * x_j,  w_2 * a + x_j')
         b <- b - step * phi_k'(w_b * a - w_x * x_j', w_2 * b - x_j)
    (the identity part carries the derivative with respect to early nodes to the end: nothing vanishes), then a cost
    term, an equality row and an inequality row that all hang on the last a and b."""
    w_b, w_x, step, w_2 = consts
    x = [p.decision_variable(float(v)) for v in start]
    a, b = x[0], x[1 % n]
    k = first_op
    for i in range(L):
        xj, xk = x[i % n], x[(i + 1) % n]
        a = a + step * _apply(m, CHAIN_OPS[k % len(CHAIN_OPS)], w_b * b + w_x * xj, w_2 * a + xk)
        k += 1
        b = b - step * _apply(m, CHAIN_OPS[k % len(CHAIN_OPS)], w_b * a - w_x * xk, w_2 * b - xj)
        k += 1
    return x, a * b, (a - b) * x[0] - 0.1, a * a + b + 2.0


def chain_start(n, stage=0):
    return [0.35 + 0.2 * j + 0.03 * stage for j in range(n)]


def _constants(m, parameters):
    if parameters is None:
        return CHAIN_CONSTANTS, []
    params = [m.variable(float(v)) for v in parameters]
    return params, params


def _assemble(m, components, parameters=None):
    """components: [(n, L, stages)] — `stages` structurally identical components each."""
    p = model.NlpProblem(m)
    consts, params = _constants(m, parameters)
    x, x0, cost, eqs, ineqs = [], [], None, [], []
    chain_cost_taken = False
    for n, L, stages in components:
        for s in range(stages):
            start = chain_start(n, s)
            xs, c, e, i = _component(m, p, n, L, start, consts)
            x += xs
            x0 += start
            # The sum of the cost joins what its terms hang on into one component (tape_compiler.cpp: nodes joined
            # through interior operands).  So one component alone, the first that is no stage of a family, gives the
            # cost its a * b; every other one gives a term on its leaves, and stays a component — and a task — of its own.
            if stages == 1 and not chain_cost_taken:
                chain_cost_taken = True
            else:
                c = 0.5 * (xs[0] * xs[0])
            cost = c if cost is None else cost + c
            eqs.append(e)
            ineqs.append(i)
    p.minimize(cost)
    for e in eqs:
        p.eq(e, 0.0)
    for i in ineqs:
        p.ge(i, 0.0)
    return TapeModel(p, x, x0, params)


def chain_model(m, n, L, stages=1, parameters=None):
    """`stages` components of L updates on n variables each.  parameters: four values that take the place of
    CHAIN_CONSTANTS as free variables that are no decision variables (as in param_models.py)."""
    return _assemble(m, [(n, L, stages)], parameters)


# The sizes of the task classes (asserted by the tests through HostCheck.info: a moved threshold fails there).
CHAIN_SIZES = {"small": (4, 4, 1), "large": (4, 12, 1), "global": (4, 40, 1), "family": (3, 4, 12)}


def mixed_model(m, with_global=True):
    """The 12-stage family, one large component and one global component in one problem: the family's generated body,
    the large task interpreted and the global kernel beside them.  Without the global component the generated launch
    has 256-thread workgroups and the large task rides in it (tape_jit.cpp: block_threads)."""
    comps = [CHAIN_SIZES["family"], CHAIN_SIZES["large"]]
    if with_global:
        comps.append(CHAIN_SIZES["global"])
    return _assemble(m, comps)


def state(tm, batch, seed, spread=0.05):
    """`batch` states (x, s, y, z) around the model's start: x within +-spread, multipliers of both signs away from 0."""
    n, me, mi = tm.dims
    rng = np.random.default_rng(seed)
    x = tm.x0[None, :] + spread * rng.uniform(-1, 1, (batch, n))
    y = rng.uniform(0.5, 1.5, (batch, me)) * rng.choice([-1.0, 1.0], (batch, me))
    z = rng.uniform(0.5, 1.5, (batch, mi))
    s = rng.uniform(0.5, 1.5, (batch, mi))
    return x, s, y, z


# ---- ops_model -------------------------------------------------------------------------------------------------------
OPS_BATCH = 32
OPS = ["ADD", "SUB", "NEG", "MUL", "DIV", "POW", "ABS", "SIGN", "SQRT", "CBRT", "EXP", "LOG", "LOG10", "SIN", "COS", "TAN",
       "ASIN", "ACOS", "ATAN", "ATAN2", "SINH", "COSH", "TANH", "ERF", "HYPOT", "MAX", "MIN", "ISNONNEG", "ISPOS"]
PIECEWISE = {"ABS", "SIGN", "MAX", "MIN", "ISNONNEG", "ISPOS"}

# Regular points: (low, high) of u and of v, inside the domain and away from the singularities and from where the
# formulas of tape_ops.h lose bits (1 / sqrt(1 - l^2) near +-1, 1 / cos^2 near pi / 2, cancellation near a zero).
WIDE, POS = (-3.0, 3.0), (0.3, 3.0)
REGULAR = {
    "ADD": (WIDE, WIDE), "SUB": (WIDE, WIDE), "NEG": (WIDE, WIDE), "MUL": (WIDE, WIDE), "DIV": (POS, POS), "POW": (POS, POS),
    "ABS": (WIDE, WIDE), "SIGN": (WIDE, WIDE), "SQRT": (POS, POS), "CBRT": (POS, POS), "EXP": (WIDE, WIDE), "LOG": (POS, POS),
    "LOG10": (POS, POS), "SIN": (WIDE, WIDE), "COS": (WIDE, WIDE), "TAN": ((-1.2, 1.2), (-1.2, 1.2)),
    "ASIN": ((-0.7, 0.7), (-0.7, 0.7)), "ACOS": ((-0.7, 0.7), (-0.7, 0.7)), "ATAN": (WIDE, WIDE), "ATAN2": ((0.3, 0.9), (1.8, 3.0)),
    "SINH": (WIDE, WIDE), "COSH": (WIDE, WIDE), "TANH": (WIDE, WIDE), "ERF": (WIDE, WIDE), "HYPOT": ((1.0, 2.0), (1.0, 2.0)),
    "MAX": (WIDE, WIDE), "MIN": (WIDE, WIDE), "ISNONNEG": (WIDE, WIDE), "ISPOS": (WIDE, WIDE),
}
# the constant child of a binary op's rows phi(u, c) and phi(c, v): (c as the right child, c as the left child)
OPS_CONSTANTS = {"ADD": (1.25, -0.75), "SUB": (1.25, -0.75), "MUL": (1.25, -0.75), "DIV": (1.25, -0.75), "POW": (3.0, 1.7),
                 "ATAN2": (0.8, -1.1), "HYPOT": (0.8, -1.1), "MAX": (0.5, 0.5), "MIN": (0.5, 0.5)}

NZ = -0.0
# Special points (u, v) of an op, taken by the LAST instances of the batch.  "extreme": a finite result that the
# reference gives to 50 digits, compared like a regular point.  "edge": compared by NaN / inf pattern and, for the
# piecewise ops, exactly.
EXTREME = {
    "SIN": [(1e5, 1e10), (-1e10, -1e5)], "COS": [(1e5, 1e10), (-1e10, -1e5)], "TAN": [(1e5, 1e10), (-1e10, -1e5)],
    "TANH": [(20.0, -20.0)], "ERF": [(20.0, -20.0)], "EXP": [(700.0, -700.0), (-700.0, 700.0)],
    "CBRT": [(-2.0, -0.3), (-27.0, 8.0), (0.37, 2.9), (1.3, 0.71), (-1.9, 5.3), (11.0, -0.052)],
    "ATAN2": [(1.0, 2.0), (1.0, -2.0), (-1.0, -2.0), (-1.0, 2.0), (0.0, 1.5), (1.5, 0.0), (0.0, -1.5), (-1.5, 0.0)],
    "POW": [(-1.5, 2.0)],  # phi(u, 3) = (-1.5)^3 with the exponent constant; the rows with a variable exponent are NaN
}
EDGE = {
    "ABS": [(0.0, NZ), (NZ, 0.0)], "SIGN": [(0.0, NZ), (NZ, 0.0)], "ISNONNEG": [(0.0, NZ), (NZ, 0.0)],
    "ISPOS": [(0.0, NZ), (NZ, 0.0)],
    "MAX": [(0.0, NZ), (NZ, 0.0), (1.5, 1.5), (0.5, 2.0), (2.0, 0.5), (0.5, 0.5)],
    "MIN": [(0.0, NZ), (NZ, 0.0), (1.5, 1.5), (0.5, 2.0), (2.0, 0.5), (0.5, 0.5)],
    "SQRT": [(0.0, 1.0)], "POW": [(0.0, 2.0), (-1.5, 2.5)], "HYPOT": [(0.0, 0.0)], "LOG": [(1e-300, 1.0)],
    "ASIN": [(1.0, -1.0)], "ACOS": [(1.0, -1.0)],
}


class OpsModel(TapeModel):
    """rows_eq / rows_ineq: per row (op, left variable index or None, right variable index or None); points (B, n);
    kind[b][op]: "regular", "extreme" or "edge"."""


def _well_rounded_cbrt_argument(rng, low, high):
    import ctypes
    import ctypes.util

    import mpmath

    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.cbrt.restype, libm.cbrt.argtypes = ctypes.c_double, [ctypes.c_double]
    while True:
        x = rng.uniform(low, high)
        c = libm.cbrt(x)
        with mpmath.workdps(50):
            if abs(mpmath.mpf(c) - mpmath.cbrt(mpmath.mpf(x))) <= 0.5 * float(np.spacing(c)):
                return x


def ops_points(seed=20260101):
    rng = np.random.default_rng(seed)
    B = OPS_BATCH
    pts = np.zeros((B, 2 * len(OPS)))
    kind = [dict() for _ in range(B)]
    for k, op in enumerate(OPS):
        special = [(p, "extreme") for p in EXTREME.get(op, [])] + [(p, "edge") for p in EDGE.get(op, [])]
        assert len(special) <= B // 2
        (ul, uh), (vl, vh) = REGULAR[op]
        for b in range(B):
            j = b - (B - len(special))
            if j >= 0:
                (pts[b, 2 * k], pts[b, 2 * k + 1]), kind[b][op] = special[j]
            else:
                pts[b, 2 * k], pts[b, 2 * k + 1] = rng.uniform(ul, uh), rng.uniform(vl, vh)
                if op == "CBRT":
                    # The second derivative of cbrt goes like v^-5: it takes an error of libm's cbrt (up to 1.8 ulp at a
                    # general argument) to 12 ulp, more than a regular point may show.  Its regular points are
                    # arguments at which libm rounds cbrt correctly (asked of libm and mpmath, not of the code under
                    # test); general arguments of both signs are among its extreme points.
                    pts[b, 2 * k], pts[b, 2 * k + 1] = (_well_rounded_cbrt_argument(rng, ul, uh) for _ in range(2))
                kind[b][op] = "regular"
    return pts, kind


def ops_model(m):
    """Per opcode k a pair (u_k, v_k) of its own.  Unary: rows phi(u), phi(v) and the inequality row phi(u) - phi(v).
    Binary: rows phi(u, v), phi(u, c), phi(c, v) — a constant child turns want_dr / want_dl off — and the inequality row
    phi(v, u).  The cost is linear: every second derivative in H is a row's."""
    p = model.NlpProblem(m)
    pts, kind = ops_points()
    x, rows_eq, rows_ineq, eqs, ineqs = [], [], [], [], []
    cost = None
    for k, op in enumerate(OPS):
        u, v = p.decision_variable(pts[0, 2 * k]), p.decision_variable(pts[0, 2 * k + 1])
        x += [u, v]
        cost = u + 0.5 * v if cost is None else cost + u + 0.5 * v
        if op in BINARY:
            cr, cl = OPS_CONSTANTS[op]
            eqs += [m._bi(op, u, v), m._bi(op, u, cr), m._bi(op, cl, v)]
            rows_eq += [(op, 2 * k, 2 * k + 1), (op, 2 * k, None), (op, None, 2 * k + 1)]
            ineqs.append(m._bi(op, v, u))
            rows_ineq.append((op, 2 * k + 1, 2 * k))
        else:
            eqs += [m._un(op, u), m._un(op, v)]
            rows_eq += [(op, 2 * k, None), (op, 2 * k + 1, None)]
            ineqs.append(m._un(op, u) - m._un(op, v))
            rows_ineq.append((op, 2 * k, 2 * k + 1))
    p.minimize(cost)
    for e in eqs:
        p.eq(e, 0.0)
    for i in ineqs:
        p.ge(i, 0.0)
    tm = OpsModel(p, x, pts[0])
    tm.rows_eq, tm.rows_ineq, tm.points, tm.kind = rows_eq, rows_ineq, pts, kind
    return tm


def ops_state(tm, seed=5):
    """(x, s, y, z) of the B instances: the points, multipliers of both signs away from 0."""
    n, me, mi = tm.dims
    rng = np.random.default_rng(seed)
    B = OPS_BATCH
    y = rng.uniform(0.5, 1.5, (B, me)) * rng.choice([-1.0, 1.0], (B, me))
    z = rng.uniform(0.5, 1.5, (B, mi))
    return tm.points.copy(), np.ones((B, mi)), y, z


DOUBLE_MAX = float(np.finfo(np.float64).max)


def ops_classify(tm, block, key):
    """(op, quantity) of an entry of instance-independent position: quantity in "value", "dl", "dr", "d2", "cost"."""
    if block in ("f", "g"):
        return None, "cost"
    if block in ("c_e", "c_i"):
        return (tm.rows_eq if block == "c_e" else tm.rows_ineq)[key][0], "value"
    if block in ("A_e", "A_i"):
        op, lv, rv = (tm.rows_eq if block == "A_e" else tm.rows_ineq)[key[0]]
        assert key[1] in (lv, rv), (block, key, op)
        return op, "dl" if key[1] == lv or op not in BINARY else "dr"
    assert key[0] // 2 == key[1] // 2, key  # H: no entry couples two ops
    return OPS[key[1] // 2], "d2"


def ops_compare(tm, b, ev, got):
    """One implementation's blocks `got` of instance b against the evaluation `ev` of the reference (mpref.Evaluation).

    Returns (measured, pattern).  measured: {(op, quantity, "regular" | "extreme"): worst error in ulps} over the entries
    of regular and extreme points where the reference is finite; an ulp is the spacing of doubles at M(e), the entry without cancellation (for
    a value or a first partial that is the entry itself).  pattern: {(block, key): (value, op, T as a double or None)}
    of every other entry — the edge points and whatever is NaN or beyond the doubles in the reference: compared between
    implementations by their NaN / inf pattern and, for the piecewise ops, exactly."""
    from . import mpref

    measured, pattern = {}, {}
    for block in mpref.BLOCKS:
        T, M = ev.T[block], ev.M[block]
        items = got[block].items() if isinstance(got[block], dict) else enumerate(got[block])
        for key, v in items:
            v = float(v)
            op, quantity = ops_classify(tm, block, key)
            t = T.get(key, mpref.ZERO) if isinstance(T, dict) else T[key]
            mag = M.get(key, mpref.ZERO) if isinstance(M, dict) else M[key]
            finite = bool(mpref.mp.isfinite(t) and mpref.mp.isfinite(mag) and mag < DOUBLE_MAX)
            kind = "regular" if op is None else tm.kind[b][op]
            if kind == "edge" or not finite:
                pattern[(block, key)] = (v, op, float(t) if finite else None)
                continue
            if v == t:
                err = 0.0
            elif not math.isfinite(v) or mag == 0:
                err = math.inf
            else:
                err = float(abs(mpref.mpf(v) - t) / mpref.mpf(float(np.spacing(float(mag)))))
            measured[(op, quantity, kind)] = max(measured.get((op, quantity, kind), 0.0), err)
    return measured, pattern


def same_pattern(a, b):
    """Two doubles of an edge entry: both NaN, the same infinity, or both finite."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return True


# ---- the cases of both tiers -----------------------------------------------------------------------------------------
# name: (builder, what HostCheck.info and tape_jit_compiles() must say: large tasks, global tasks, shared tasks, bodies)
CASES = {
    "small": (lambda m: chain_model(m, *CHAIN_SIZES["small"]), (0, 0, 0, 0)),
    "large": (lambda m: chain_model(m, *CHAIN_SIZES["large"]), (1, 0, 0, 0)),
    "global": (lambda m: chain_model(m, *CHAIN_SIZES["global"]), (0, 1, 0, 0)),
    "family": (lambda m: chain_model(m, *CHAIN_SIZES["family"]), (0, 0, 11, 1)),
    "mixed": (lambda m: mixed_model(m), (1, 1, 11, 1)),
    "ride": (lambda m: mixed_model(m, with_global=False), (1, 0, 11, 1)),
}
ACCURACY_BATCH = 2
STATE_SEED = 3


def task_class(hc):
    """(large tasks, global tasks, shared tasks, generated bodies) of a HostCheck."""
    return (hc.info["tape_large_tasks"], hc.info["tape_global_tasks"], hc.info["tape_shared_tasks"], hc.tape_jit_compiles())


_measured = {}


def measure(name):
    """The CPU side of a case, computed once per process: the states, the reference's evaluations, and the host
    interpreter and the oracle against them.  Builds and closes its own models: call it BEFORE building a model of
    the test's own (the expression arenas are shared) — the result holds numbers only.

    chain cases: {"class", "scaling_is_one", "state", "evs", "host": [compare() per instance], "oracle": [...],
    "rho_host", "rho_oracle": {block: worst}};
    "ops": {"class", "state", "evs", "host", "oracle": {(op, quantity, kind): ulps}, "host_pattern", "oracle_pattern":
    [per instance {(block, key): (value, op, T)}]}."""
    if name in _measured:
        return _measured[name]
    import sleipnir_amd

    from . import hostcheck, mpref, oracle, parity

    sleipnir_amd.lib().slpx_graph_reset()
    oracle.lib().orc_reset()
    make = ops_model if name == "ops" else CASES[name][0]
    prod = make(model.Model(model.ProductBackend("hostcheck")))
    orc = make(model.Model(model.OracleBackend()))
    ref = make(model.Model(mpref.MpBackend()))
    hc = hostcheck.HostCheck(prod.p.p)
    out = {"class": task_class(hc), "scaling_is_one": bool(np.all(orc.p.p.scaling() == 1.0)), "dims": prod.dims}
    x, s, y, z = ops_state(prod) if name == "ops" else state(prod, ACCURACY_BATCH, STATE_SEED)
    out["state"] = (x, s, y, z)
    out["evs"] = [ref.p.p.evaluate(x[b], y[b], z[b]) for b in range(len(x))]
    host_blocks, oracle_blocks = [], []
    for b in range(len(x)):
        host_blocks.append(parity.unpack_sweep(hc, hc.sweep(x[b], y[b], z[b], True)))
        orc.p.p.newton_step(x[b], s[b], y[b], z[b], 0.1, False)
        oracle_blocks.append(mpref.blocks_of_oracle(orc.p.p))
    if name == "ops":
        out["rows"] = prod
        for who, blocks in (("host", host_blocks), ("oracle", oracle_blocks)):
            worst, patterns = {}, []
            for b in range(len(x)):
                m_, p_ = ops_compare(prod, b, out["evs"][b], blocks[b])
                for k, v in m_.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                patterns.append(p_)
            out[who], out[who + "_pattern"] = worst, patterns
    else:
        for who, blocks in (("host", host_blocks), ("oracle", oracle_blocks)):
            out[who] = [mpref.compare(out["evs"][b], blocks[b]) for b in range(len(x))]
            out["rho_" + who] = mpref.worst(out[who])
    hc.close()
    prod.close()
    _measured[name] = out
    return out
