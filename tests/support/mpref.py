"""A high-precision reference for the AD sweep: a third Backend for tests/support/model.py, beside OracleBackend and
ProductBackend.  It records the expression graph in Python and evaluates it with mpmath at 50 digits by second-order
Taylor propagation: every node carries its value, its gradient and its Hessian with respect to the decision variables,
from the closed forms phi, phi', phi'' of the 31 opcodes (no symbolic differentiation, no double arithmetic: nothing in
common with the two implementations it judges).

Piecewise ops follow the reference's conventions as sleipnir_amd/csrc/tape_ops.h states them: abs'(0) = 0, sign' = 0,
max / min give the LEFT argument on a tie, ISNONNEG / ISPOS have zero derivative.

A second pass runs the same recurrences on absolute values: M(e) >= |T(e)| is what the entry e would be if nothing
cancelled.  Errors are measured as rho(e) = |V(e) - T(e)| / (2^-53 M(e)).

Outside an op's domain (log of a negative, a division by zero) a derivative is NaN here; callers compare only the
finite entries with this reference and the rest by their NaN / inf pattern between the implementations.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import math

import numpy as np
from mpmath import mp, mpf

from . import cases, model

mp.dps = 50

OPS = model.OPS
NAMES = {v: k for k, v in OPS.items()}
U = mpf(2) ** -53
NAN = mpf("nan")
ZERO, ONE = mpf(0), mpf(1)
LN10 = mp.log(10)
TWO_INV_SQRT_PI = 2 / mp.sqrt(mp.pi)
BINARY = {"ADD", "SUB", "MUL", "DIV", "POW", "ATAN2", "HYPOT", "MAX", "MIN"}
NO_DERIVATIVE = {"SIGN", "ISNONNEG", "ISPOS"}


def _real(v):
    return v if isinstance(v, mpf) else NAN


def _guard(fn):
    """phi and its derivatives outside the domain: NaN instead of an exception or a complex number."""
    try:
        return tuple(_real(v) for v in fn())
    except (ZeroDivisionError, ValueError, TypeError):
        return None


def _cbrt(l):
    return mp.cbrt(l) if l >= 0 else -mp.cbrt(-l)


def unary(name, l):
    """(phi, phi', phi'') at l."""
    if name == "NEG": return -l, -ONE, ZERO
    if name == "ABS": return abs(l), (mpf(-1) if l < 0 else (ONE if l > 0 else ZERO)), ZERO
    if name == "SIGN": return (mpf(-1) if l < 0 else (ZERO if l == 0 else ONE)), ZERO, ZERO
    if name == "ISNONNEG": return (ONE if l >= 0 else ZERO), ZERO, ZERO
    if name == "ISPOS": return (ONE if l > 0 else ZERO), ZERO, ZERO
    if name == "SQRT":
        v = mp.sqrt(l)
        return v, 1 / (2 * v), -1 / (4 * v * l)
    if name == "CBRT":
        v = _cbrt(l)
        return v, 1 / (3 * v * v), -2 * v / (9 * l * l)
    if name == "EXP":
        v = mp.exp(l)
        return v, v, v
    if name == "LOG": return mp.log(l), 1 / l, -1 / (l * l)
    if name == "LOG10": return mp.log10(l), 1 / (l * LN10), -1 / (l * l * LN10)
    if name == "SIN": return mp.sin(l), mp.cos(l), -mp.sin(l)
    if name == "COS": return mp.cos(l), -mp.sin(l), -mp.cos(l)
    if name == "TAN":
        t = mp.tan(l)
        return t, 1 + t * t, 2 * t * (1 + t * t)
    if name == "ASIN":
        w = 1 - l * l
        return mp.asin(l), 1 / mp.sqrt(w), l / (w * mp.sqrt(w))
    if name == "ACOS":
        w = 1 - l * l
        return mp.acos(l), -1 / mp.sqrt(w), -l / (w * mp.sqrt(w))
    if name == "ATAN":
        w = 1 + l * l
        return mp.atan(l), 1 / w, -2 * l / (w * w)
    if name == "SINH": return mp.sinh(l), mp.cosh(l), mp.sinh(l)
    if name == "COSH": return mp.cosh(l), mp.sinh(l), mp.cosh(l)
    if name == "TANH":
        c = mp.cosh(l)
        return mp.tanh(l), 1 / (c * c), -2 * mp.tanh(l) / (c * c)
    if name == "ERF":
        d = TWO_INV_SQRT_PI * mp.exp(-l * l)
        return mp.erf(l), d, -2 * l * d
    raise KeyError(name)


def binary_value(name, l, r):
    if name == "ADD": return l + r
    if name == "SUB": return l - r
    if name == "MUL": return l * r
    if name == "DIV": return l / r
    if name == "POW": return mp.power(l, r)
    if name == "ATAN2": return mp.atan2(l, r)
    if name == "HYPOT": return mp.hypot(l, r)
    if name == "MAX": return l if l >= r else r
    if name == "MIN": return l if l <= r else r
    raise KeyError(name)


def binary_left(name, l, r):
    """(phi_l, phi_ll): what a node needs of its left child when the right one is a constant."""
    if name in ("ADD", "SUB"): return ONE, ZERO
    if name == "MUL": return r, ZERO
    if name == "DIV": return 1 / r, ZERO
    if name == "POW": return r * mp.power(l, r - 1), r * (r - 1) * mp.power(l, r - 2)
    if name == "ATAN2":
        den = l * l + r * r
        return r / den, -2 * l * r / (den * den)
    if name == "HYPOT":
        h = mp.hypot(l, r)
        return l / h, r * r / (h * h * h)
    if name == "MAX": return (ONE if l >= r else ZERO), ZERO
    if name == "MIN": return (ONE if l <= r else ZERO), ZERO
    raise KeyError(name)


def binary_right(name, l, r):
    """(phi_r, phi_rr)."""
    if name == "ADD": return ONE, ZERO
    if name == "SUB": return -ONE, ZERO
    if name == "MUL": return l, ZERO
    if name == "DIV": return -l / (r * r), 2 * l / (r * r * r)
    if name == "POW":
        if l < 0:
            return NAN, NAN  # v log(l): NaN in the reference too
        ln = mp.log(l) if l > 0 else mpf("-inf")
        v = mp.power(l, r)
        return v * ln, v * ln * ln
    if name == "ATAN2":
        den = l * l + r * r
        return -l / den, 2 * l * r / (den * den)
    if name == "HYPOT":
        h = mp.hypot(l, r)
        return r / h, l * l / (h * h * h)
    if name == "MAX": return (ZERO if l >= r else ONE), ZERO
    if name == "MIN": return (ZERO if l <= r else ONE), ZERO
    raise KeyError(name)


def binary_cross(name, l, r):
    """phi_lr."""
    if name == "MUL": return ONE
    if name == "DIV": return -1 / (r * r)
    if name == "POW":
        if l < 0:
            return NAN
        ln = mp.log(l) if l > 0 else mpf("-inf")
        return mp.power(l, r - 1) * (1 + r * ln)
    if name == "ATAN2":
        den = l * l + r * r
        return (l * l - r * r) / (den * den)
    if name == "HYPOT":
        h = mp.hypot(l, r)
        return -l * r / (h * h * h)
    return ZERO


class Taylor:
    """value v, gradient g {var: d}, Hessian h {(i, j), i >= j: d}; mv, mg, mh: the same on absolute values."""

    __slots__ = ("v", "g", "h", "mv", "mg", "mh")

    def __init__(self, v, mv=None):
        self.v, self.g, self.h = v, {}, {}
        self.mv, self.mg, self.mh = (abs(v) if mv is None else mv), {}, {}


def _axpy(out, a, x):
    if a == 0 and not mp.isnan(a):
        # a structural zero factor (abs'(0), the losing side of max): the entries stay in the pattern with value 0
        for k in x:
            out.setdefault(k, ZERO)
        return
    for k, v in x.items():
        out[k] = out.get(k, ZERO) + a * v


def _outer(out, a, x, y, symmetric_pair):
    """out += a x y^T (lower triangle); with symmetric_pair, a (x y^T + y x^T)."""
    if a == 0 and not mp.isnan(a):
        return
    for i, xi in x.items():
        for j, yj in y.items():
            if symmetric_pair:
                k = (i, j) if i >= j else (j, i)
                out[k] = out.get(k, ZERO) + a * xi * yj * (2 if i == j else 1)
            elif i >= j:
                out[(i, j)] = out.get((i, j), ZERO) + a * xi * yj


def _combine(t, A, B, dl, dr, dll, dlr, drr, field_g, field_h):
    g, h = getattr(t, field_g), getattr(t, field_h)
    if A is not None:
        ga, ha = getattr(A, field_g), getattr(A, field_h)
        _axpy(g, dl, ga)
        _axpy(h, dl, ha)
        _outer(h, dll, ga, ga, False)
    if B is not None:
        gb, hb = getattr(B, field_g), getattr(B, field_h)
        _axpy(g, dr, gb)
        _axpy(h, dr, hb)
        _outer(h, drr, gb, gb, False)
    if A is not None and B is not None:
        _outer(h, dlr, getattr(A, field_g), getattr(B, field_g), True)


class MpProblem:
    """What model.NlpProblem needs of a problem: decision variables, a cost, rows."""

    def __init__(self, be):
        self.be = be
        self.x, self.cost, self.eq, self.ineq = [], None, [], []

    def decision_variable(self):
        node = self.be.var(0.0)
        self.x.append(node)
        return node

    def minimize(self, node): self.cost = node
    def subject_to_eq(self, node): self.eq.append(node)
    def subject_to_ineq(self, node): self.ineq.append(node)

    @property
    def dims(self):
        return len(self.x), len(self.eq), len(self.ineq)

    def close(self):
        pass

    def evaluate(self, x, y=None, z=None, values=None):
        return Evaluation(self, x, y, z, values)


class MpBackend(model.Backend):
    name = "mpref"

    def __init__(self):
        self.nodes = []  # (opcode name, a, b, value of a leaf)

    def reset(self):
        self.nodes = []

    def new_problem(self):
        return MpProblem(self)

    def _add(self, rec):
        self.nodes.append(rec)
        return len(self.nodes) - 1

    def var(self, value=0.0): return self._add(["VAR", -1, -1, float(value)])
    def const(self, value): return self._add(["CONST", -1, -1, float(value)])
    def unary(self, op, a): return self._add([NAMES[op], a, -1, None])
    def binary(self, op, a, b): return self._add([NAMES[op], a, b, None])

    def set_value(self, i, v):
        assert self.nodes[i][0] == "VAR"
        self.nodes[i][3] = float(v)

    def value(self, i):
        name, a, b, leaf = self.nodes[i]
        if leaf is not None:
            return leaf
        if name in BINARY:
            return float(binary_value(name, mpf(self.value(a)), mpf(self.value(b))))
        return float(unary(name, mpf(self.value(a)))[0])


class Evaluation:
    """The graph of `problem` at x (and, for H, the multipliers y, z): T and M of every block.

    values: {node: value} for variables that are no decision variables (parameters); theirs default to the node's own."""

    def __init__(self, problem, x, y=None, z=None, values=None):
        be = problem.be
        n, me, mi = problem.dims
        index = {node: i for i, node in enumerate(problem.x)}
        x = [mpf(float(v)) for v in x]
        values = values or {}
        done = {}
        roots = [r for r in [problem.cost] + problem.eq + problem.ineq if r is not None]
        # nodes are created children first: ascending order is a topological order
        needed, stack = set(), list(roots)
        while stack:
            i = stack.pop()
            if i in needed:
                continue
            needed.add(i)
            _, a, b, _ = be.nodes[i]
            stack.extend(c for c in (a, b) if c >= 0)
        for i in sorted(needed):
            name, a, b, leaf = be.nodes[i]
            if name == "VAR" and i in index:
                t = Taylor(x[index[i]])
                t.g[index[i]] = ONE
                t.mg[index[i]] = ONE
            elif name in ("VAR", "CONST"):
                t = Taylor(mpf(float(values.get(i, leaf))))
            else:
                t = self._node(name, done[a], done[b] if b >= 0 else None)
            done[i] = t
        self.n, self.m_e, self.m_i = n, me, mi
        self.nodes = done
        cost = done[problem.cost] if problem.cost is not None else Taylor(ZERO)
        eq, ineq = [done[r] for r in problem.eq], [done[r] for r in problem.ineq]
        y = [mpf(float(v)) for v in (np.zeros(me) if y is None else y)]
        z = [mpf(float(v)) for v in (np.zeros(mi) if z is None else z)]
        self.T, self.M = {}, {}
        for out, fv, fg, fh in ((self.T, "v", "g", "h"), (self.M, "mv", "mg", "mh")):
            mag = out is self.M
            out["f"] = [getattr(cost, fv)]
            out["c_e"] = [getattr(t, fv) for t in eq]
            out["c_i"] = [getattr(t, fv) for t in ineq]
            out["g"] = {(c, 0): v for c, v in getattr(cost, fg).items()}
            out["A_e"] = {(r, c): v for r, t in enumerate(eq) for c, v in getattr(t, fg).items()}
            out["A_i"] = {(r, c): v for r, t in enumerate(ineq) for c, v in getattr(t, fg).items()}
            # the Lagrangian of the reference: L = f - y^T c_e - z^T c_i
            H = {}
            _axpy(H, ONE, getattr(cost, fh))
            for mult, rows in ((y, eq), (z, ineq)):
                for w, t in zip(mult, rows):
                    _axpy(H, abs(w) if mag else -w, getattr(t, fh))
            out["H"] = H

    @staticmethod
    def _node(name, A, B):
        l = A.v
        if B is None:
            res = _guard(lambda: unary(name, l))
            if res is None:
                v = _guard(lambda: (unary_value_only(name, l),))
                res = (v[0] if v else NAN, NAN, NAN)
            v, d1, d2 = res
            t = Taylor(v)
            if name in NO_DERIVATIVE or not A.g:
                return t
            _combine(t, A, None, d1, None, d2, None, None, "g", "h")
            _combine(t, A, None, abs(d1), None, abs(d2), None, None, "mg", "mh")
            return t
        r = B.v
        v = _guard(lambda: (binary_value(name, l, r),))
        v = v[0] if v else NAN
        # value magnitude: through the linear ops what the value would be without cancellation, |v| elsewhere
        if name in ("ADD", "SUB"):
            mv = A.mv + B.mv
        elif name == "MUL":
            mv = A.mv * B.mv
        else:
            mv = abs(v)
        t = Taylor(v, mv)
        left, right = bool(A.g), bool(B.g)
        dl = dll = dr = drr = dlr = ZERO
        if left:
            res = _guard(lambda: binary_left(name, l, r))
            dl, dll = res if res else (NAN, NAN)
        if right:
            res = _guard(lambda: binary_right(name, l, r))
            dr, drr = res if res else (NAN, NAN)
        if left and right:
            res = _guard(lambda: (binary_cross(name, l, r),))
            dlr = res[0] if res else NAN
        _combine(t, A if left else None, B if right else None, dl, dr, dll, dlr, drr, "g", "h")
        _combine(t, A if left else None, B if right else None, abs(dl), abs(dr), abs(dll), abs(dlr), abs(drr), "mg", "mh")
        return t


def unary_value_only(name, l):
    """phi alone where a derivative is outside its domain (sqrt(0), asin(1))."""
    if name == "SQRT": return mp.sqrt(l)
    if name == "CBRT": return _cbrt(l)
    if name == "ASIN": return mp.asin(l)
    if name == "ACOS": return mp.acos(l)
    return unary(name, l)[0]


# ---- an implementation's V against T ---------------------------------------------------------------------------------
BLOCKS = ("f", "c_e", "c_i", "g", "A_e", "A_i", "H")


def blocks_of_oracle(op):
    """The oracle's evaluation (after op.newton_step(..., do_solve=False)) in the layout of parity.unpack_sweep; its g
    is dense: a column the cost does not depend on is an entry that must be exactly 0."""
    out = {"f": np.array([op.f()]), "c_e": op.vec("c_e"), "c_i": op.vec("c_i")}
    out["g"] = {(c, 0): v for c, v in enumerate(op.vec("g"))}
    for name in ("A_e", "A_i", "H"):
        cp, ri, val = op.csc(name)
        out[name] = cases.csc_to_dict(cp, ri, val)
    return out


def _entries(got):
    """(key, value) of every stored entry of an implementation's block."""
    if isinstance(got, dict):
        return list(got.items())
    return [(k, float(v)) for k, v in enumerate(got)]


def compare(ev, got):
    """rho per block of one implementation's blocks `got` against the evaluation `ev`, entry by entry.

    Returns {block: {"rho": worst rho over the finite entries of T, "count": entries compared, "nonfinite": keys where T
    is not finite, "tmin" / "tmax": range of |T| over the compared nonzero entries}}.  Asserts that no entry is left
    out: every entry the implementation stores is compared, and every entry of T it does not store is a true zero."""
    res = {}
    for block in BLOCKS:
        T, M = ev.T[block], ev.M[block]
        as_dict = isinstance(T, dict)
        worst, count, nonfinite, tmin, tmax = 0.0, 0, [], math.inf, 0.0
        seen = set()
        for key, v in _entries(got[block]):
            seen.add(key)
            t = T.get(key, ZERO) if as_dict else T[key]
            m = M.get(key, ZERO) if as_dict else M[key]
            if not mp.isfinite(t) or not mp.isfinite(m):
                nonfinite.append(key)
                continue
            count += 1
            if not math.isfinite(v):
                worst = math.inf
                continue
            err = abs(mpf(v) - t)
            if err == 0:
                rho = 0.0
            elif m == 0:
                rho = math.inf
            else:
                rho = float(err / (U * m))
            worst = max(worst, rho)
            if t != 0:
                tmin, tmax = min(tmin, float(abs(t))), max(tmax, float(abs(t)))
        if as_dict:
            for key, t in T.items():
                if key not in seen:
                    # (a sparse pattern may drop what is identically zero, nothing else)
                    assert t == 0 and M[key] == 0, (block, key, "an entry of the reference that the implementation does not store")
        res[block] = {"rho": worst, "count": count, "nonfinite": nonfinite, "tmin": tmin, "tmax": tmax}
    return res


def worst(results):
    """Blockwise maximum of rho over several compare() results."""
    return {b: max(r[b]["rho"] for r in results) for b in BLOCKS}
