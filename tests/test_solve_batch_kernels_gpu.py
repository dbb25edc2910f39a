"""The batched interior-point kernels (ipm_batch_kernels.h) through their launch wrappers (BatchIpmDevice,
ipm_batch_launch.hip), instance by instance: a probe (tests/support/batchcheck.cpp) drives each method on the batch
system of a model (`sa.System(problem, B)`: tape at unit scales, as Problem::batch_system builds it), and every output
is compared with plain float64 numpy of the same formulas (interior_point.hpp, kkt_error.hpp, as batch_lockstep.cpp
consumes them).  Each instance of a batch has its own scales, iterate, mu, tau, step sizes and flags, and the mask of
active instances has holes.  The V of instance b is taken from a batch-1 system of the same model under that instance's
scales (its V is pinned to the oracle by test_gpu_parity.py).

Tolerances:
  * V after the per-instance scaling (batch_scale_V_kernel), c_e, c_i of a trial point, V at the fallback's full step:
    bit for bit against the batch-1 system (both paths apply one multiplication per entry);
  * min, max, fraction-to-the-boundary, counts, copies and the z clamp of commit: exact;
  * sums (norms, dot products, A^T v, right-hand sides, the correction's p_s, p_z): 1e-12 of the sum of the terms'
    magnitudes (numpy sums in np.longdouble);
  * the trial point x + alpha p: at most the rounding of the product alpha p apart (the device may contract it into an
    FMA; numpy does not), plus the sum's own ulp;
  * the solve: the device's p against a dense numpy solve of the instance's assembled, regularized KKT matrix, at
    1e-9 relative, or 1e-14 times the matrix's condition number where that is larger;
  * everything of one instance is bit for bit the same at slot 0 of B=1, slot 5 of B=7 and slot 129 of B=130, whatever
    the other instances and the mask are.
"""
from __future__ import annotations

import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import batchcheck as bc
from tests.support import cases, model, models

pytestmark = pytest.mark.gpu

ERR = bc.ERR
KAPPA = 1e10
SENTINEL = 7.25  # what every slot of an inactive instance holds before a method call, and must hold after it
# the per-instance buffers an inactive instance's slot must keep: the iterate, the trial point, the correction and its
# accumulators (and m_out, checked per call).  m_Vcur and the system's V are excluded: the sweeps run every instance of
# the batch, active or not, and so do the assembly of the system's lhs / rhs and its solve.  So are p, p_s, p_z:
# newton_direction takes the system's whole solution in one copy.
KEPT = ["x", "s", "y", "z", "tx", "ts", "ty", "tz", "sx", "ss", "sy", "sz", "tce", "tci", "sce", "scims"]


# ---------------------------------------------------------------- models

def _rosenbrock(m):  # n = 2, m_e = 0, m_i = 2: the dense LDL^T branch
    p = model.NlpProblem(m)
    x, y = p.decision_variable(-1.2), p.decision_variable(0.8)
    p.minimize(100 * m.pow(y - m.pow(x, 2), 2) + m.pow(1 - x, 2))
    p.ge(y, m.pow(x - 1, 3) + 1)
    p.le(y, -x + 2)
    return p.p


def _small_mixed(m):  # n = 3, m_e = 2, m_i = 2 (test_solve_batch_gpu.py: test_restoration_inside_a_batch)
    p = model.NlpProblem(m)
    x, s1, s2 = p.decision_variable(-2), p.decision_variable(3), p.decision_variable(1)
    p.minimize(x)
    p.eq(m.pow(x, 2) - s1 - 1, 0)
    p.eq(x - s2 - 0.5, 0)
    p.ge(s1, 0)
    p.ge(s2, 0)
    return p.p


SHAPES = {
    "rosenbrock": lambda m: _rosenbrock(m),
    "small_mixed": lambda m: _small_mixed(m),
    "flywheel_50": lambda m: models.flywheel(50, 0.005),        # sizes between 64 and 256
    "cart_pole_100": lambda m: models.cart_pole(100, 0.05),     # above 256; separable cost (partial sums in V's tail)
}

_rigs = {}


class Rig:
    """One model: its batch systems with their probes, and the batch-1 reference system."""

    def __init__(self, name):
        m = model.Model(model.ProductBackend("gpu"))
        self.name = name
        self.problem = SHAPES[name](m)
        self.ref = sa.System(self.problem, 1)
        info = self.ref.info
        self.n, self.me, self.mi, self.nV = info["n"], info["m_e"], info["m_i"], info["nV"]
        self.off = dict(f=0, ce=1, ci=1 + self.me, g=info["off_g"], Ae=info["off_Ae"], Ai=info["off_Ai"])
        self.tail = self.nV - (info["off_Hc"] + info["nnz_Hc"])
        g_cp, _ = self.ref.pattern(0)
        self.g_src = np.full(self.n, -1)
        for c in range(self.n):
            if g_cp[c + 1] > g_cp[c]:
                self.g_src[c] = info["off_g"] + g_cp[c]
        self.Ae = self._csc(1, info["off_Ae"], self.me)
        self.Ai = self._csc(2, info["off_Ai"], self.mi)
        self.lhs_pat = self.ref.pattern(5)
        self.x0 = self.problem.get_x()
        self.systems = {}

    def _csc(self, which, off, rows):
        cp, ri = self.ref.pattern(which)
        cols = np.repeat(np.arange(self.n), np.diff(cp))
        return dict(ri=ri.astype(np.int64), cols=cols, idx=off + np.arange(len(ri)), rows=rows)

    def probe(self, B):
        if B not in self.systems:
            system = sa.System(self.problem, B)
            self.systems[B] = (system, bc.BatchProbe(system))
        return self.systems[B][1]

    # ---- numpy on one instance ----
    def g(self, V):
        return np.where(self.g_src >= 0, V[np.maximum(self.g_src, 0)], 0.0)

    def At(self, A, V, v, vals=None):
        """(A^T v) in long double, and the sum of the terms' magnitudes"""
        terms = np.asarray(V[A["idx"]] if vals is None else vals, dtype=np.longdouble) * np.asarray(v)[A["ri"]]
        out, mag = np.zeros(self.n, dtype=np.longdouble), np.zeros(self.n, dtype=np.longdouble)
        np.add.at(out, A["cols"], terms)
        np.add.at(mag, A["cols"], np.abs(terms))
        return out, mag

    def Ai_rows(self, V, px):
        """A_i p_x per row, and the magnitudes"""
        A = self.Ai
        terms = np.asarray(V[A["idx"]], dtype=np.longdouble) * np.asarray(px)[A["cols"]]
        out, mag = np.zeros(self.mi, dtype=np.longdouble), np.zeros(self.mi, dtype=np.longdouble)
        np.add.at(out, A["ri"], terms)
        np.add.at(mag, A["ri"], np.abs(terms))
        return out, mag

    def V_ref(self, scales, x, s=None, y=None, z=None, full=True):
        """V of the batch-1 system under `scales` at the point"""
        self.ref.set_scaling(scales)
        if full:
            self.ref.set_state(x, s, y, z)
        else:
            self.ref.set_state(x=x)
        self.ref.sweep(full)
        return self.ref.get("V")[0]


def rig(name):
    if name not in _rigs:
        _rigs[name] = Rig(name)
    return _rigs[name]


@pytest.fixture(scope="module")
def probes():
    """(the module's own fixture of the probe: a fresh arena for its models, the probe library built)"""
    sa.lib().slpx_graph_reset()
    bc.lib()
    yield rig
    for r in _rigs.values():
        for system, probe in r.systems.values():
            probe.close()
            system.close()
        r.ref.close()
        r.problem.close()
    _rigs.clear()
    sa.lib().slpx_graph_reset()


# ---------------------------------------------------------------- instances

def instance(r, k):
    """Instance k of model r: everything of it depends on k alone (not on its slot or its batch)."""
    rng = np.random.default_rng(cases.SEED + 7919 * k)
    n, me, mi = r.n, r.me, r.mi
    scales = np.concatenate([[rng.uniform(0.2, 1.0)], rng.uniform(0.2, 1.0, me), rng.uniform(0.2, 1.0, mi)])
    x, s, y, z, _ = cases.newton_state("interior", r.x0, n, me, mi, scales[0], seed=cases.SEED + k)
    if k % 4 == 3:
        x = x + 20.0  # far from the start: violated inequality rows, c_i <= 0
    elif k % 4 == 2:
        x = x - 20.0
    if k % 5 == 1:
        y = 1e3 * y   # a large multiplier: an indefinite Hessian of the Lagrangian, regularized
    return dict(scales=scales, x=x, s=s, y=y, z=z, mu=scales[0] * 10.0 ** rng.uniform(-3, -0.5),
                tau=rng.uniform(0.99, 0.9999), s_from_ci=k % 2, frac=rng.uniform(0.3, 0.9),
                frac_z=rng.uniform(0.3, 0.9), soc1=rng.uniform(0.2, 1.0), soc2=rng.uniform(0.2, 1.0),
                delta0=[0.0, 1e-4, 3e-3][k % 3], gamma0=[0.0, 1e-10, 1e-9][k % 3],
                positive_step=k % 7 == 4)  # the direction's p_s made positive: alpha_max = 1


def step_close(dev, x, a, p):
    """dev = x + a p up to the rounding of the product a p, which a fused multiply-add skips (and the sum's own)"""
    prod = a * np.asarray(p)
    ref = x + prod
    return np.all(np.abs(dev - ref) <= np.spacing(np.abs(prod)) + np.spacing(np.abs(ref)))


def sum_close(dev, ref, mag, rel=1e-12):
    dev, ref, mag = (np.asarray(v, dtype=np.float64) for v in (dev, ref, mag))
    return np.all(np.abs(dev - ref) <= rel * np.maximum(mag, np.abs(ref)) + 1e-300)


def ftb(x, p, tau):
    m = p < 0
    return min(1.0, float(np.min(-tau / p[m] * x[m]))) if m.any() else 1.0


def lsum(v):
    v = np.asarray(v, dtype=np.longdouble)
    return float(v.sum()), float(np.abs(v).sum())


# ---------------------------------------------------------------- the numpy reference

def ref_errors(r, V, x, s, y, z, sc, mu):
    """batch_errors_kernel's 29 values: (value, kind, magnitude) with kind 'exact', 'sum' or 'either' (a product
    feeding a subtraction, which the device may contract: the plain and the fused rounding both pass)"""
    me, mi = r.me, r.mi
    d_f, d_ce, d_ci = sc[0], sc[1:1 + me], sc[1 + me:]
    inv_f = 1.0 / d_f
    ce, ci, g = V[r.off["ce"]:r.off["ce"] + me], V[r.off["ci"]:r.off["ci"] + mi], r.g(V)
    aey, aey_m = r.At(r.Ae, V, y)
    aiz, aiz_m = r.At(r.Ai, V, z)
    d = g - aey - aiz
    d_mag = np.abs(g) + aey_m + aiz_m
    yu, zu, su = d_ce * y * inv_f, d_ci * z * inv_f, (1.0 / d_ci) * s
    aeu, aeu_m = r.At(r.Ae, V, yu, vals=(1.0 / d_ce[r.Ae["ri"]]) * V[r.Ae["idx"]])
    aiu, aiu_m = r.At(r.Ai, V, zu, vals=(1.0 / d_ci[r.Ai["ri"]]) * V[r.Ai["idx"]])
    du = inv_f * g - aeu - aiu
    du_mag = np.abs(inv_f * g) + aeu_m + aiu_m
    aec, aec_m = r.At(r.Ae, V, ce)
    cm = np.minimum(ci, 0.0)
    aic, aic_m = r.At(r.Ai, V, cm)
    e = {}
    mx = lambda v: float(np.max(v)) if len(v) else 0.0
    e["F"] = (V[r.off["f"]], "exact", 0)
    e["DUAL_INF"] = (mx(np.abs(d)), "sum", mx(d_mag))
    e["DUAL_1"] = (float(np.abs(d).sum()), "sum", float(d_mag.sum()))
    e["Y1"] = (lsum(np.abs(y))[0], "sum", lsum(np.abs(y))[0])
    e["Z1"] = (lsum(np.abs(z))[0], "sum", lsum(np.abs(z))[0])
    sz = s * z
    e["SZ_MAX"] = (max(0.0, mx(sz)), "exact", 0)
    e["SZ_MIN"] = (float(np.min(sz)) if mi else np.inf, "exact", 0)
    e["COMP_1"] = (lsum(np.abs(sz - mu))[0], "sum", lsum(np.abs(sz) + mu)[0])
    e["CE_INF"] = (mx(np.abs(ce)), "exact", 0)
    e["CE_1"] = (lsum(np.abs(ce))[0], "sum", lsum(np.abs(ce))[0])
    e["CIS_INF"] = (mx(np.abs(ci - s)), "exact", 0)
    e["CIS_1"] = (lsum(np.abs(ci - s))[0], "sum", lsum(np.abs(ci - s))[0])
    e["DUALU_INF"] = (mx(np.abs(du)), "sum", mx(du_mag))
    e["YU1"] = (lsum(np.abs(yu))[0], "sum", lsum(np.abs(yu))[0])
    e["ZU1"] = (lsum(np.abs(zu))[0], "sum", lsum(np.abs(zu))[0])
    e["COMPU_INF"] = (mx(np.abs(su * zu)), "exact", 0)
    e["CEU_INF"] = (mx(np.abs((1.0 / d_ce) * ce)), "exact", 0)
    e["CISU_INF"] = (mx(np.abs((1.0 / d_ci) * ci - su)), "either", ((1.0 / d_ci), ci, su))
    e["LOGSUM"] = (lsum(np.log(s))[0], "sum", lsum(np.abs(np.log(s)))[0])
    e["V_BAD"] = (float(np.sum(~np.isfinite(V))), "exact", 0)
    e["CI_NONPOS"] = (float(np.sum(~(ci > 0.0))), "exact", 0)
    e["AETCE2"] = (lsum(np.asarray(aec, dtype=np.float64) ** 2)[0], "sum", lsum(np.asarray(aec_m, dtype=np.float64) ** 2)[0])
    e["CE2"] = (lsum(ce ** 2)[0], "sum", lsum(ce ** 2)[0])
    e["AITCM2"] = (lsum(np.asarray(aic, dtype=np.float64) ** 2)[0], "sum", lsum(np.asarray(aic_m, dtype=np.float64) ** 2)[0])
    e["CM2"] = (lsum(cm ** 2)[0], "sum", lsum(cm ** 2)[0])
    e["X_INF"] = (mx(np.abs(x)), "exact", 0)
    e["X_BAD"] = (float(np.sum(~np.isfinite(x))), "exact", 0)
    e["S_INF"] = (mx(np.abs(s)), "exact", 0)
    e["S_BAD"] = (float(np.sum(~np.isfinite(s))), "exact", 0)
    return e


def _fma_max_abs(a, b, c):
    """max |a b - c| with a b - c rounded once (exact rational arithmetic)"""
    from fractions import Fraction
    best = 0.0
    for ai, bi, ci in zip(a, b, c):
        best = max(best, abs(float(Fraction(float(ai)) * Fraction(float(bi)) - Fraction(float(ci)))))
    return best


def check_errors(r, dev, ref, what):
    bad = []
    for k, (val, kind, mag) in ref.items():
        got = dev[ERR[k]]
        if kind == "exact":
            ok = got == val or (np.isnan(got) and np.isnan(val))
        elif kind == "sum":
            ok = sum_close(got, val, mag)
        else:
            ok = got == val or got == _fma_max_abs(*mag)
        if not ok:
            bad.append((k, got, val))
    assert not bad, f"{r.name} {what}: {bad}"


# ---------------------------------------------------------------- the scenario: every method in the driver's order

def scenario(r, B, ids, active, nan_tz=None):
    """Runs every BatchIpmDevice method on a batch of instances `ids` (slot b holds instance ids[b]) with the mask
    `active`, inactive slots filled with SENTINEL, and records every output and buffer after every call.  Checks that no
    call touched an inactive slot of KEPT or of its own output.  nan_tz = (slot, row): that trial z is NaN at the commit."""
    pr = r.probe(B)
    inst = [instance(r, k) for k in ids]
    act = np.asarray(active, dtype=np.uint8)
    on = act.astype(bool)
    n, me, mi = r.n, r.me, r.mi

    def stack(key, width):
        return np.array([inst[b][key] if on[b] else np.full(width, SENTINEL) for b in range(B)]).reshape(B, width)

    pr.set_scales(np.array([i["scales"] for i in inst]))
    for name in KEPT:
        pr.put(name, np.full(pr.get(name).size, SENTINEL))
    pr.set_iterate(stack("x", n), stack("s", mi), stack("y", me), stack("z", mi))
    col = lambda key: np.array([i[key] for i in inst], dtype=np.float64)
    mu, tau = col("mu"), col("tau")
    rec = {"ids": list(ids), "active": act}

    def params(**kw):
        base = dict(mu=mu, tau=tau, alpha=np.ones(B), alpha_z=np.ones(B), alpha_soc=np.ones(B), mode=np.zeros(B),
                    s_from_ci=col("s_from_ci"), first=np.zeros(B), active=act)
        base.update(kw)
        pr.set_params(**base)

    def call(tag, fn, width=None):
        before = {name: pr.get(name) for name in KEPT}
        pr.put("out", np.full(B * len(bc.ERR_KEYS), SENTINEL))
        out = fn()
        for name in KEPT:
            after = pr.get(name)
            assert np.array_equal(after[~on], before[name][~on]), f"{r.name} B={B} {tag}: an inactive slot of {name}"
        if out is not None:
            for o in out if isinstance(out, tuple) else (out,):
                assert np.all(o[~on] == SENTINEL), f"{r.name} B={B} {tag}: an inactive slot of the output"
        rec[tag] = out
        rec[tag + ":buf"] = {name: pr.get(name) for name in KEPT + ["Vcur", "p", "ps", "pz"]}
        return out

    # scaling and refresh; the same iterate again
    params()
    call("refresh", pr.refresh)
    rec["sys_syz"] = [pr.get(k) for k in ("sys_s", "sys_y", "sys_z")]
    call("refresh2", pr.refresh)
    # the Newton system and its masked, speculative compute from each instance's delta / gamma memory
    pr.assemble()
    rec["lhs"], rec["rhs"] = pr.get("sys_lhs"), pr.get("sys_rhs")
    d0, g0 = col("delta0"), col("gamma0")
    pr.set_regularization(d0, g0)
    info, _ = pr.compute(True, act)
    rec["info"], rec["reg"], rec["reg0"] = info, pr.regularization(), (d0, g0)
    rec["sys_p"] = pr.get("sys_p")
    # a direction with no negative p_s for some instances (alpha_max exactly 1)
    ps, pzs = pr.get("sys_ps"), pr.get("sys_pz")
    for b in range(B):
        if on[b] and inst[b]["positive_step"]:
            ps[b] = np.abs(ps[b])
    pr.put("sys_ps", ps)
    dirs = call("direction", pr.newton_direction)
    amax = np.where(on, dirs[:, 0], 1.0)
    az = np.where(on, dirs[:, 1], 1.0)
    # trial point along the Newton direction at per-instance step sizes, with and without s_from_ci
    alpha, alpha_z = col("frac") * amax, col("frac_z") * az
    params(alpha=alpha, alpha_z=alpha_z)
    call("trial", pr.trial_values)
    # two rounds of second-order corrections, each followed by its trial point
    params(alpha_soc=col("soc1"), first=np.ones(B))
    rec["soc1:rhs_before"] = pr.get("sce"), pr.get("scims")
    sd1 = call("soc1", pr.soc_step)
    rec["soc1:sys"] = (pr.get("sys_rhs"), pr.get("sys_p"))
    params(alpha=np.where(on, sd1[:, 0], 1.0), alpha_z=np.where(on, sd1[:, 1], 1.0), mode=np.ones(B))
    call("trial_soc1", pr.trial_values)
    params(alpha_soc=col("soc2"), first=np.zeros(B))
    sd2 = call("soc2", pr.soc_step)
    rec["soc2:sys"] = (pr.get("sys_rhs"), pr.get("sys_p"))
    params(alpha=np.where(on, sd2[:, 0], 1.0), alpha_z=np.where(on, sd2[:, 1], 1.0), mode=np.ones(B))
    call("trial_soc2", pr.trial_values)
    # refresh -> trial_values -> refresh: the current point's V and errors come back
    params()
    call("refresh3", pr.refresh)
    # the KKT-error fallback at the full step (s_from_ci set for some instances: the method clears it)
    params(alpha=amax, alpha_z=az, s_from_ci=np.ones(B))
    call("fallback", pr.kkt_fallback)
    rec["fallback:V"] = pr.get("sys_V")
    rec["fallback:s_from_ci"] = pr.s_from_ci()
    # commit, with trial z below, above and between the clamp's bounds
    tz, ts = pr.get("tz"), pr.get("ts")
    for b in range(B):
        if on[b] and mi:
            lo, hi = 1.0 / KAPPA * mu[b] / ts[b], KAPPA * mu[b] / ts[b]
            j = np.arange(mi) % 3
            tz[b] = np.where(j == 0, 0.5 * lo, np.where(j == 1, 2.0 * hi, np.sqrt(lo * hi)))
    if nan_tz is not None:
        tz[nan_tz[0]][nan_tz[1]] = np.nan
    pr.put("tz", tz)
    params()
    call("commit", pr.commit)
    rec["inst"] = inst
    return rec


MASKS = {
    1: lambda: np.ones(1, dtype=np.uint8),
    7: lambda: np.array([1, 1, 0, 1, 1, 0, 1], dtype=np.uint8),
    130: lambda: (np.random.default_rng(130).uniform(size=130) < 0.7).astype(np.uint8) | (np.arange(130) == 129),
}


# ---------------------------------------------------------------- the checks of one scenario

def check_scenario(r, rec, slots):
    n, me, mi = r.n, r.me, r.mi
    tag = lambda b: f"{r.name} B={len(rec['ids'])} slot {b} (instance {rec['ids'][b]})"
    for b in slots:
        i = rec["inst"][b]
        sc, x, s, y, z, mu, tau = (i[k] for k in ("scales", "x", "s", "y", "z", "mu", "tau"))
        # 1. scaling and refresh
        Vc = rec["refresh:buf"]["Vcur"][b]
        Vr = r.V_ref(sc, x, s, y, z)
        assert np.array_equal(Vc, Vr), (tag(b), np.flatnonzero(Vc != Vr)[:10])
        assert np.array_equal(rec["refresh2:buf"]["Vcur"][b], Vc) and np.array_equal(rec["refresh2"][b], rec["refresh"][b])
        assert np.array_equal(rec["refresh3:buf"]["Vcur"][b], Vc) and np.array_equal(rec["refresh3"][b], rec["refresh"][b])
        for buf, v in zip(rec["sys_syz"], (s, y, z)):
            assert np.array_equal(buf[b], v), tag(b)
        check_errors(r, rec["refresh"][b], ref_errors(r, Vr, x, s, y, z, sc, mu), tag(b) + " refresh")
        # 2. the solve of the Newton system: a dense solve of the regularized matrix
        delta, gamma = rec["reg"][0][b], rec["reg"][1][b]
        assert rec["info"][b] == 0, tag(b)
        check_solve(r, rec["lhs"][b], rec["rhs"][b], rec["sys_p"][b], delta, gamma, tag(b) + " Newton step")
        # 3. direction
        p, ps, pz = (rec["direction:buf"][k][b] for k in ("p", "ps", "pz"))
        assert np.array_equal(p, rec["sys_p"][b])
        if i["positive_step"]:
            assert np.all(ps >= 0) and rec["direction"][b][0] == 1.0, tag(b)
        d = rec["direction"][b]
        assert d[0] == ftb(s, ps, tau) and d[1] == ftb(z, pz, tau), (tag(b), d)
        gp, gp_m = lsum(r.g(Vr) * p[:n])
        lb, lb_m = lsum((1.0 / s) * ps)
        assert sum_close(d[2], gp - mu * lb, gp_m + mu * lb_m), (tag(b), d[2], gp - mu * lb)
        # 4. trial point along the Newton direction
        a, az = i["frac"] * d[0], i["frac_z"] * d[1]
        tb = rec["trial:buf"]
        check_trial(r, rec["trial"][b], tb, b, sc, x, s, y, z, p[:n], ps, -p[n:], pz, a, az,
                    s_from_ci=bool(i["s_from_ci"]), tag=tag(b) + " trial")
        # 5. second-order corrections
        Vcur = Vr
        ce, ci = Vcur[r.off["ce"]:r.off["ce"] + me], Vcur[r.off["ci"]:r.off["ci"] + mi]
        prev_ce, prev_cims, trial_buf = ce, ci - s, tb
        for rnd, soc_a in ((1, i["soc1"]), (2, i["soc2"])):
            sb = rec[f"soc{rnd}:buf"]
            rhs, psol = (v[b] for v in rec[f"soc{rnd}:sys"])
            tce, tci, ts = trial_buf["tce"][b], trial_buf["tci"][b], trial_buf["ts"][b]
            sce_ref = soc_a * prev_ce + tce
            scims_ref = soc_a * prev_cims + tci - ts
            assert sum_close(sb["sce"][b], sce_ref, np.abs(soc_a * prev_ce) + np.abs(tce)), (tag(b), rnd)
            assert sum_close(sb["scims"][b], scims_ref, np.abs(soc_a * prev_cims) + np.abs(tci) + np.abs(ts)), (tag(b), rnd)
            sce, scims = sb["sce"][b], sb["scims"][b]
            t = mu * (1.0 / s) - ((1.0 / s) * z) * scims
            aey, aey_m = r.At(r.Ae, Vcur, y)
            ait, ait_m = r.At(r.Ai, Vcur, t)
            gx = r.g(Vcur)
            assert sum_close(rhs[:n], -gx + aey + ait, np.abs(gx) + aey_m + ait_m), (tag(b), rnd)
            assert np.array_equal(rhs[n:], -sce), (tag(b), rnd)
            check_solve(r, rec["lhs"][b], rhs, psol, delta, gamma, f"{tag(b)} correction {rnd}")
            assert np.array_equal(sb["sx"][b], psol[:n]) and np.array_equal(sb["sy"][b], -psol[n:]), (tag(b), rnd)
            aipx, aipx_m = r.Ai_rows(Vcur, psol[:n])
            assert sum_close(sb["ss"][b], scims + aipx, np.abs(scims) + aipx_m), (tag(b), rnd)
            ss = sb["ss"][b]
            pz_ref = mu * (1.0 / s) - z - ((1.0 / s) * z) * ss
            assert sum_close(sb["sz"][b], pz_ref, mu / s + z + np.abs((1.0 / s) * z * ss)), (tag(b), rnd)
            sdv = rec[f"soc{rnd}"][b]
            assert sdv[0] == ftb(s, ss, tau) and sdv[1] == ftb(z, sb["sz"][b], tau), (tag(b), rnd, sdv)
            trial_buf = rec[f"trial_soc{rnd}:buf"]
            check_trial(r, rec[f"trial_soc{rnd}"][b], trial_buf, b, sc, x, s, y, z, sb["sx"][b], ss, sb["sy"][b],
                        sb["sz"][b], sdv[0], sdv[1], s_from_ci=False, tag=f"{tag(b)} trial of correction {rnd}")
            prev_ce, prev_cims = sce, scims
        # 6. KKT-error fallback: errors at the current point, then at the full step
        cur, tri = rec["fallback"]
        assert np.array_equal(cur[b], rec["refresh"][b]), tag(b)
        fb = rec["fallback:buf"]
        tx, ts, ty, tz = (fb[k][b] for k in ("tx", "ts", "ty", "tz"))
        assert step_close(tx, x, d[0], p[:n]) and step_close(ts, s, d[0], ps), tag(b)
        assert step_close(ty, y, d[1], -p[n:]) and step_close(tz, z, d[1], pz), tag(b)
        Vt = r.V_ref(sc, tx, ts, ty, tz)
        assert np.array_equal(rec["fallback:V"][b], Vt), (tag(b), np.flatnonzero(rec["fallback:V"][b] != Vt)[:10])
        check_errors(r, tri[b], ref_errors(r, Vt, tx, ts, ty, tz, sc, mu), tag(b) + " fallback's full step")
        assert not rec["fallback:s_from_ci"].any()
        # 7. commit
        cb = rec["commit:buf"]
        assert np.array_equal(cb["x"][b], tx) and np.array_equal(cb["s"][b], ts) and np.array_equal(cb["y"][b], ty)
        tz = rec["commit:buf"]["tz"][b]
        assert np.array_equal(cb["z"][b], z_reset(tz, mu, ts)), tag(b)


def z_reset(tz, mu, ts):
    """interior_point.hpp:797-801, std::clamp(z, mu / (kappa s), kappa mu / s) as its two comparisons"""
    lo, hi = 1.0 / KAPPA * mu / ts, KAPPA * mu / ts
    return np.where(tz < lo, lo, np.where(tz > hi, hi, tz))


def check_trial(r, met, tb, b, sc, x, s, y, z, px, ps, py, pz, a, az, s_from_ci, tag):
    n, me, mi = r.n, r.me, r.mi
    tx, ts, ty, tz, tce, tci = (tb[k][b] for k in ("tx", "ts", "ty", "tz", "tce", "tci"))
    assert step_close(tx, x, a, px), tag
    assert step_close(ty, y, az, py) and step_close(tz, z, az, pz), tag
    Vt = r.V_ref(sc, tx, full=False)
    ce, ci = Vt[r.off["ce"]:r.off["ce"] + me], Vt[r.off["ci"]:r.off["ci"] + mi]
    assert np.array_equal(tce, ce) and np.array_equal(tci, ci), tag
    if s_from_ci:
        assert np.array_equal(ts, ci), tag
    else:
        assert step_close(ts, s, a, ps), tag
    assert met[0] == Vt[r.off["f"]], tag
    viol, viol_m = lsum(np.concatenate([np.abs(ce), np.abs(ci - ts)]))
    assert sum_close(met[1], viol, viol_m), (tag, met[1], viol)
    with np.errstate(invalid="ignore"):
        logs = np.log(ts)
    ls, ls_m = lsum(logs)
    assert sum_close(met[2], ls, ls_m) or (np.isnan(met[2]) and np.isnan(ls)), (tag, met[2], ls)
    bad = np.sum(~np.isfinite(ce)) + np.sum(~np.isfinite(ci)) + (0 if np.isfinite(Vt[0]) else 1)
    assert met[3] == bad, tag


def check_solve(r, lhs, rhs, p, delta, gamma, tag):
    cp, ri = r.lhs_pat
    dim = r.n + r.me
    K = cases.lower_csc_to_dense_sym(cp, ri, cases.regularized(cp, ri, lhs, r.n, delta, gamma), dim)
    p_ref = np.linalg.solve(K, rhs)
    err = np.max(np.abs(p - p_ref)) / max(np.max(np.abs(p_ref)), 1e-300)
    if err > 1e-9:  # (an ill-conditioned instance: the bound grows with the condition number)
        cond = np.linalg.cond(K)
        assert err <= max(1e-9, 1e-14 * cond), (tag, err, cond)


# ---------------------------------------------------------------- tests

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("B", [7, 130])
def test_every_phase_against_numpy(probes, shape, B):
    r = probes(shape)
    rec = scenario(r, B, list(range(B)), MASKS[B]())
    on = np.flatnonzero(rec["active"])
    slots = on if B <= 7 else on[np.linspace(0, len(on) - 1, 6).astype(int)]
    check_scenario(r, rec, slots)
    if B == 7:
        errs = rec["refresh"][on]
        # the batch mixes instances with and without c_i <= 0 rows, with and without regularization
        assert (errs[:, ERR["CI_NONPOS"]] > 0).any() and (errs[:, ERR["CI_NONPOS"]] == 0).any()
        assert (errs[:, ERR["AITCM2"]] > 0).any()
        if r.me:
            assert (errs[:, ERR["AETCE2"]] > 0).all()
    if shape == "cart_pole_100":
        assert r.tail > 0  # (the cost's partial sums in V's hidden tail are part of the V compared)
        assert (rec["reg"][0][on] > 0).any()


def test_commit_leaves_a_nan_trial_z_as_solve_does(probes):
    """The z reset of the commit is solve()'s and the reference's, std::clamp: neither of its comparisons holds for a
    NaN, which therefore stays (fmin / fmax would turn it into the lower end).  Instance 3 of seven gets a NaN in one
    trial z at the commit: that entry is NaN afterwards, the rest of the instance is what it is without the NaN, and so
    is every other instance, bit for bit."""
    r = probes("small_mixed")
    B, slot, j = 7, 3, 1
    mask = MASKS[B]()
    assert mask[slot] and r.mi == 2
    plain = scenario(r, B, list(range(B)), mask)
    hit = scenario(r, B, list(range(B)), mask, nan_tz=(slot, j))
    for name in KEPT:
        assert np.array_equal(hit["fallback:buf"][name], plain["fallback:buf"][name]), name
    cb, cp = hit["commit:buf"], plain["commit:buf"]
    assert np.isnan(cb["tz"][slot][j]) and not np.isnan(cp["tz"]).any()
    for name in KEPT:
        if name in ("z", "tz"):
            continue
        assert np.array_equal(cb[name], cp[name]), name
    others = np.arange(B) != slot
    assert np.array_equal(cb["z"][others], cp["z"][others])
    assert not np.isnan(cp["z"]).any()
    assert np.isnan(cb["z"][slot][j])
    keep = np.arange(r.mi) != j
    assert np.array_equal(cb["z"][slot][keep], cp["z"][slot][keep])
    mu = hit["inst"][slot]["mu"]
    assert np.array_equal(cb["z"][slot], z_reset(cb["tz"][slot], mu, cb["s"][slot]), equal_nan=True)


def test_masked_compute(probes):
    """compute(true, mask): the active instances get what an unmasked compute and a batch-1 compute from the same state
    and delta / gamma memory give them; the others keep their memory."""
    for shape in ("cart_pole_100", "rosenbrock", "small_mixed"):
        r = probes(shape)
        B = 7
        mask = MASKS[B]()
        pr = r.probe(B)
        inst = [instance(r, k) for k in range(B)]
        d0 = np.array([i["delta0"] for i in inst])
        g0 = np.array([i["gamma0"] for i in inst])
        pr.set_scales(np.array([i["scales"] for i in inst]))
        pr.set_iterate(*(np.array([i[k] for i in inst]) for k in ("x", "s", "y", "z")))
        # the unmasked compute of the whole batch at the refreshed point
        pr.set_params(mu=np.array([i["mu"] for i in inst]))
        pr.refresh()
        pr.assemble()
        lhs_m, rhs_m = pr.get("sys_lhs"), pr.get("sys_rhs")
        pr.set_regularization(d0, g0)
        info_all, _ = pr.compute(True)
        reg_all, p_all = pr.regularization(), pr.get("sys_p")
        # the masked one
        pr.set_regularization(d0, g0)
        info_m, _ = pr.compute(True, mask)
        reg_m, p_m = pr.regularization(), pr.get("sys_p")
        on = mask.astype(bool)
        assert np.array_equal(info_m[on], info_all[on]) and (info_m[~on] == 0).all()
        assert np.array_equal(reg_m[0][on], reg_all[0][on]) and np.array_equal(reg_m[1][on], reg_all[1][on])
        assert np.array_equal(reg_m[0][~on], d0[~on]) and np.array_equal(reg_m[1][~on], g0[~on]), shape
        assert np.array_equal(p_m[on], p_all[on]), shape
        # batch-1 computes of the active instances from the same state and memory
        one = r.probe(1)
        for b in np.flatnonzero(on):
            i = inst[b]
            one.set_scales(i["scales"])
            one.set_iterate(i["x"], i["s"], i["y"], i["z"])
            one.set_params(mu=[i["mu"]])
            one.refresh()
            one.assemble()
            one.set_regularization([i["delta0"]], [i["gamma0"]])
            info1, _ = one.compute(True, np.ones(1))
            reg1 = one.regularization()
            assert info1[0] == info_m[b] and reg1[0][0] == reg_m[0][b] and reg1[1][0] == reg_m[1][b], (shape, b)
            # (a batch-1 system factors with the single-problem LDL^T plan, newton.cpp: the same system solved in another
            # order — the solution at the solve's tolerance)
            check_solve(r, one.get("sys_lhs")[0], one.get("sys_rhs")[0], one.get("sys_p")[0], reg1[0][0], reg1[1][0],
                        f"{shape} batch-1 compute of instance {b}")
            assert np.array_equal(one.get("sys_lhs")[0], lhs_m[b]) and np.array_equal(one.get("sys_rhs")[0], rhs_m[b])
        if shape == "cart_pole_100":
            assert (reg_m[0][on] > 0).any()  # (regularized instances among them)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_an_instance_is_independent_of_its_slot_batch_and_mask(probes, shape):
    """Instance K at slot 0 of B=1, slot 5 of B=7 and slot 129 of B=130, under different masks and among different
    instances (and no inactive slot touched: scenario checks that on every call).  Within one batch size every output
    and buffer of K is the same to the bit at any slot, under any mask.  Across batch sizes it is up to the solve: the
    LDL^T plan is chosen by the batch size (newton.cpp: the single-problem plan for B=1, task sizes for a small batch,
    the interleaved layout for a large one), each summing in its own order — so from the solve on, each run of K is
    checked against numpy instead."""
    r = probes(shape)
    K = 4  # (an instance with a positive p_s: alpha_max = 1)
    runs = {}
    for B, slot, flip in ((1, 0, False), (7, 5, False), (7, 1, True), (130, 129, False), (130, 5, True)):
        ids = list(range(100, 100 + B))
        ids[slot] = K
        mask = MASKS[B]()
        if flip:  # (another mask: the complement)
            mask = 1 - mask
        mask[slot] = 1
        rec = scenario(r, B, ids, mask)
        check_scenario(r, rec, [slot])
        runs[(B, slot)] = rec
    up_to_solve = ("refresh", "refresh2", "lhs", "rhs", "info")
    ref0 = runs[(1, 0)]
    for (B, slot), rec in runs.items():
        for key in up_to_solve:
            assert np.array_equal(rec[key][slot], ref0[key][0]), (shape, key, B, slot)
        assert np.array_equal(rec["refresh:buf"]["Vcur"][slot], ref0["refresh:buf"]["Vcur"][0]), (shape, B, slot)
        assert rec["reg"][0][slot] == ref0["reg"][0][0] and rec["reg"][1][slot] == ref0["reg"][1][0], (shape, B, slot)
    for B, (s0, s1) in ((7, (5, 1)), (130, (129, 5))):
        rec0, rec, slot0, slot = runs[(B, s0)], runs[(B, s1)], s0, s1
        for key, val in rec0.items():
            if key in ("ids", "active", "inst", "reg0", "fallback:s_from_ci") or val is None:
                continue
            other = rec[key]
            if key.endswith(":buf"):
                for name, buf in val.items():
                    if name in ("p", "ps", "pz") and key.startswith("refresh"):
                        continue  # (not yet taken from the solve: what an earlier run left)
                    assert np.array_equal(other[name][slot], buf[slot0]), (shape, B, key, name)
            elif key == "reg":
                assert other[0][slot] == val[0][slot0] and other[1][slot] == val[1][slot0], (shape, B)
            elif isinstance(val, (tuple, list)):
                for a, b in zip(other, val):
                    assert np.array_equal(a[slot], b[slot0]), (shape, B, key)
            else:
                assert np.array_equal(other[slot], val[slot0]), (shape, B, key)


def test_nonfinite_values_stay_in_their_instance(probes):
    r = probes("flywheel_50")
    B = 7
    pr = r.probe(B)
    inst = [instance(r, k) for k in range(B)]
    X = np.array([i["x"] for i in inst])
    S, Y, Z = (np.array([i[k] for i in inst]) for k in ("s", "y", "z"))
    mu = np.array([i["mu"] for i in inst])
    pr.set_scales(np.array([i["scales"] for i in inst]))

    def run(x, alpha):
        pr.set_iterate(x, S, Y, Z)
        pr.set_params(mu=mu)
        err = pr.refresh()
        pr.assemble()
        pr.set_regularization(np.zeros(B), np.zeros(B))
        pr.compute(True, np.ones(B))
        pr.newton_direction()
        pr.set_params(mu=mu, alpha=alpha, alpha_z=0.5 * np.ones(B))
        met = pr.trial_values()
        return err, met, pr.get("tx"), pr.get("tci")

    alpha = np.full(B, 0.5)
    err, met, tx, tci = run(X, alpha)
    Xn = X.copy()
    Xn[2, 3] = np.nan
    alpha_inf = alpha.copy()
    alpha_inf[4] = np.inf  # the trial point of instance 4 leaves the finite numbers
    err_n, met_n, tx_n, tci_n = run(Xn, alpha_inf)
    assert err_n[2, ERR["X_BAD"]] == 1.0 and err_n[2, ERR["V_BAD"]] > 0
    assert met_n[4, 3] > 0
    for b in range(B):
        if b in (2, 4):
            continue
        assert np.array_equal(err_n[b], err[b], equal_nan=True) and np.array_equal(met_n[b], met[b], equal_nan=True), b
        assert np.array_equal(tx_n[b], tx[b]) and np.array_equal(tci_n[b], tci[b]), b
    assert err[:, ERR["X_BAD"]].sum() == 0 and err[:, ERR["V_BAD"]].sum() == 0
