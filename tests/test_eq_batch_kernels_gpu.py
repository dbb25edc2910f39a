"""The kernels of the batched SQP / Newton drivers (eq_batch_kernels.h, and batch_errors_kernel as they call it with
m_i = 0) through their launch wrappers (BatchEqDevice), one at a time: a probe (tests/support/eqbatchcheck.cpp) drives
each method on the batch system of a model at B = 3 with the middle instance inactive, and every output is compared
with plain float64 / long double numpy of the same formulas on the downloaded buffers.  Two models: the two-variable
circle (dense branch, one pass of the 256 threads) and the pendulum chain at N = 100 (n = 302 crosses 256 threads,
m_e = 204 does not: both loop shapes).

Tolerances:
  * copies, negations, products of two doubles, maxima of such entries (|c_e|_inf, its unscaled form, |x|_inf), counts
    and flags, f: exact;
  * sums (one-norms, squared two-norms, dot products, A_e^T v, right-hand sides) and the maxima over such sums
    (|g - A_e^T y|_inf): 1e-12 of the sum of the terms' magnitudes (numpy sums in np.longdouble);
  * a + alpha b (trial points, the correction's accumulator): the rounding of the product apart at most (the device may
    contract it into an FMA), plus the sum's own ulp.
The inactive instance's slices of every per-instance buffer of BatchEqDevice (iterate, trial point, both directions,
the correction's accumulators, the output block) are compared byte for byte before and after each call.  Its slices
of the current point's V and of the system's own buffers are not: the sweeps, the assembly and the solve run every
instance of the batch, and refresh keeps the whole V in one copy."""
import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import eq_models, eqbatchcheck as ebc, model

pytestmark = pytest.mark.gpu

ERR = ebc.ERR
EPS = np.finfo(np.float64).eps
KEPT = ["x", "y", "tx", "ty", "px", "py", "sx", "sy", "tce", "sce"]
ACTIVE = np.array([1, 0, 1], dtype=np.uint8)
B = 3


class Rig:
    def __init__(self, name, m):
        self.problem = (eq_models.circle(m) if name == "circle" else eq_models.pendulum(m)).p
        self.system = sa.System(self.problem, B)
        self.pr = ebc.EqBatchProbe(self.system)
        info = self.system.info
        self.n, self.me, self.nV = info["n"], info["m_e"], info["nV"]
        assert (self.n, self.me) == ((2, 1) if name == "circle" else (302, 204)) and info["m_i"] == 0
        self.off_ce, self.off_g = 1, info["off_g"]
        g_cp, _ = self.system.pattern(0)
        self.g_src = np.full(self.n, -1)
        for c in range(self.n):
            if g_cp[c + 1] > g_cp[c]:
                self.g_src[c] = self.off_g + g_cp[c]
        cp, ri = self.system.pattern(1)
        self.Ae = dict(ri=ri.astype(np.int64), cols=np.repeat(np.arange(self.n), np.diff(cp)),
                       idx=info["off_Ae"] + np.arange(len(ri)))
        rng = np.random.default_rng(11 + self.n)
        self.S = rng.uniform(0.5, 2.0, (B, 1 + self.me))
        self.x = (np.array([[0.7, 0.9], [1.3, 0.4], [0.2, 1.1]]) if name == "circle"
                  else 0.3 * rng.standard_normal((B, self.n)))
        self.y = rng.standard_normal((B, self.me))
        self.rng = rng

    def g(self, V):
        return np.where(self.g_src >= 0, V[np.maximum(self.g_src, 0)], 0.0)

    def At(self, V, v):
        """(A_e^T v) in long double, and the sum of the terms' magnitudes"""
        A = self.Ae
        terms = np.asarray(V[A["idx"]], dtype=np.longdouble) * np.asarray(v)[A["ri"]]
        out, mag = np.zeros(self.n, dtype=np.longdouble), np.zeros(self.n, dtype=np.longdouble)
        np.add.at(out, A["cols"], terms)
        np.add.at(mag, A["cols"], np.abs(terms))
        return out, mag

    def start(self):
        """scales, iterate, distinct junk in every other kept buffer, all active -> refresh"""
        pr = self.pr
        pr.set_scales(self.S)
        pr.set_iterate(self.x, self.y)
        for k, name in enumerate(KEPT[2:]):
            shape = pr.get(name).shape
            pr.put(name, 3.0 + k + self.rng.standard_normal(shape))
        pr.set_params(active=ACTIVE)

    def call(self, fn, per_out=0):
        """fn() with the inactive instance's slices compared byte for byte before and after"""
        pr = self.pr
        before = {k: pr.get(k)[1].copy() for k in KEPT}
        out_before = pr.get("out").reshape(-1)[per_out:2 * per_out].copy()
        r = fn()
        for k in KEPT:
            assert before[k].tobytes() == pr.get(k)[1].tobytes(), k
        assert out_before.tobytes() == pr.get("out").reshape(-1)[per_out:2 * per_out].tobytes()
        return r


@pytest.fixture(scope="module")
def rigs(slpx, orc):
    """both models in one expression arena, emptied once for the module"""
    orc.lib().orc_reset()
    be = model.ProductBackend("gpu")
    be.reset()
    return {"m": model.Model(be)}


@pytest.fixture(params=["circle", "pendulum"])
def rig(request, rigs):
    if request.param not in rigs:
        rigs[request.param] = Rig(request.param, rigs["m"])
    r = rigs[request.param]
    r.start()
    return r


def _close(dev, ref, mag, what):
    assert abs(float(dev) - float(ref)) <= 1e-12 * float(mag) + 1e-300, (what, dev, float(ref), float(mag))


def _check_errors(r, e, V, x, y, S, what):
    """one instance's row of batch_errors_kernel against numpy (kkt_error.hpp, scaled and un-scaled)"""
    ld = np.longdouble
    inv_f = 1.0 / S[0]
    sc = S[1:]
    ce = V[r.off_ce:r.off_ce + r.me]
    g = r.g(V)
    aty, mag = r.At(V, y)
    d = g.astype(ld) - aty
    dmag = np.abs(g) + mag
    assert e[ERR["F"]] == V[0]
    k = int(np.argmax(np.abs(d)))
    _close(e[ERR["DUAL_INF"]], np.max(np.abs(d)), np.max(dmag), what + " dual inf")
    _close(e[ERR["DUAL_1"]], np.sum(np.abs(d)), np.sum(dmag), what + " dual 1")
    _close(e[ERR["DUALU_INF"]], np.max(np.abs(d)) * inv_f, np.max(dmag) * inv_f, what + " dual inf unscaled")
    _close(e[ERR["Y1"]], np.sum(np.abs(y).astype(ld)), np.sum(np.abs(y)), what + " y1")
    yu = np.abs(sc * y * inv_f)
    _close(e[ERR["YU1"]], np.sum(yu.astype(ld)), np.sum(yu), what + " y1 unscaled")
    assert e[ERR["CE_INF"]] == (np.max(np.abs(ce)) if r.me else 0.0)
    assert e[ERR["CEU_INF"]] == (np.max(np.abs((1.0 / sc) * ce)) if r.me else 0.0)
    _close(e[ERR["CE_1"]], np.sum(np.abs(ce).astype(ld)), np.sum(np.abs(ce)), what + " ce 1")
    _close(e[ERR["CE2"]], np.sum(ce.astype(ld) ** 2), np.sum(ce ** 2), what + " ce 2")
    atc, cmag = r.At(V, ce)
    _close(e[ERR["AETCE2"]], np.sum(atc ** 2), np.sum(cmag ** 2), what + " AeT ce")
    assert e[ERR["X_INF"]] == np.max(np.abs(x))
    assert e[ERR["X_BAD"]] == np.sum(~np.isfinite(x)) and e[ERR["V_BAD"]] == np.sum(~np.isfinite(V))
    for key in ("Z1", "SZ_MAX", "COMP_1", "CIS_INF", "CIS_1", "ZU1", "COMPU_INF", "CISU_INF", "LOGSUM", "CI_NONPOS",
                "AITCM2", "CM2", "S_INF", "S_BAD"):
        assert e[ERR[key]] == 0.0, key
    assert e[ERR["SZ_MIN"]] == np.inf


def _axpy_close(dev, a, alpha, b, what):
    tol = EPS * (np.abs(alpha * b) + np.abs(a + alpha * b)) + 1e-300
    assert np.all(np.abs(dev - (a + alpha * b)) <= tol), what


def test_refresh_errors(rig):
    pr = rig.pr
    err = rig.call(pr.refresh, len(ebc.ERR_KEYS))
    Vcur, sysV, sys_in, sys_y = pr.get("Vcur"), pr.get("sys_V"), pr.get("sys_in"), pr.get("sys_y")
    for b in (0, 2):
        assert np.array_equal(Vcur[b], sysV[b])
        assert np.array_equal(sys_in[b][:rig.n], rig.x[b])
        assert np.array_equal(sys_in[b][rig.n:rig.n + rig.me], rig.S[b][1:] * rig.y[b])
        assert np.array_equal(sys_y[b], rig.y[b])
        _check_errors(rig, err[b], Vcur[b], rig.x[b], rig.y[b], rig.S[b], f"refresh {b}")
    # a non-finite entry of x is counted, and its instance alone sees it
    x = rig.x.copy()
    x[2, rig.n - 1] = np.nan
    pr.set_iterate(x, rig.y)
    err2 = rig.call(pr.refresh, len(ebc.ERR_KEYS))
    assert err2[2][ERR["X_BAD"]] == 1.0 and err2[2][ERR["V_BAD"]] >= 1.0
    assert np.array_equal(err2[0], err[0])


def _stepped(rig):
    pr = rig.pr
    pr.refresh()
    info = pr.newton_step()
    assert info[0] == 0 and info[2] == 0, info
    return rig.call(pr.direction, 1)


def test_direction(rig):
    pr = rig.pr
    dphi = _stepped(rig)
    p, px, py, Vcur = pr.get("sys_p"), pr.get("px"), pr.get("py"), pr.get("Vcur")
    for b in (0, 2):
        assert np.array_equal(px[b], p[b][:rig.n]) and np.array_equal(py[b], -p[b][rig.n:])
        terms = rig.g(Vcur[b]).astype(np.longdouble) * px[b]
        _close(dphi[b], np.sum(terms), np.sum(np.abs(terms)), f"D_phi {b}")


def test_trial_point_and_metrics(rig):
    pr = rig.pr
    _stepped(rig)
    alpha = np.array([0.5, 1.0, 0.25])
    pr.set_params(alpha=alpha, active=ACTIVE)
    met = rig.call(pr.trial_values, 3)
    tx, ty, px, py, sysV, tce, sys_in = (pr.get(k) for k in ("tx", "ty", "px", "py", "sys_V", "tce", "sys_in"))
    for b in (0, 2):
        _axpy_close(tx[b], rig.x[b], alpha[b], px[b], "trial x")
        _axpy_close(ty[b], rig.y[b], alpha[b], py[b], "trial y")
        assert np.array_equal(sys_in[b][:rig.n], tx[b])
        ce = sysV[b][rig.off_ce:rig.off_ce + rig.me]
        assert np.array_equal(tce[b], ce)
        assert met[b][0] == sysV[b][0] and met[b][2] == 0.0
        _close(met[b][1], np.sum(np.abs(ce).astype(np.longdouble)), np.sum(np.abs(ce)), "trial violation")
    # a non-finite trial point is flagged: the count of non-finite f, c_e, exactly
    alpha[2] = np.inf
    pr.set_params(alpha=alpha, active=ACTIVE)
    met2 = rig.call(pr.trial_values, 3)
    sysV = pr.get("sys_V")
    bad = np.sum(~np.isfinite(sysV[2][rig.off_ce:rig.off_ce + rig.me])) + (not np.isfinite(sysV[2][0]))
    assert bad >= 1 and met2[2][2] == bad
    assert np.array_equal(met2[0], met[0])


def test_second_order_correction(rig):
    pr = rig.pr
    _stepped(rig)
    pr.set_params(alpha=np.ones(B), active=ACTIVE)
    pr.trial_values()
    Vcur, tce = pr.get("Vcur"), pr.get("tce")
    # first round: the accumulator starts from c_e; second round: from itself
    a1, a2 = np.array([1.0, 1.0, 0.75]), np.array([0.5, 1.0, 1.0])
    pr.set_params(alpha=np.ones(B), alpha_soc=a1, first=np.ones(B), active=ACTIVE)
    rig.call(pr.soc_step)
    sce1, rhs, p, sx, sy = (pr.get(k) for k in ("sce", "sys_rhs", "sys_p", "sx", "sy"))
    for b in (0, 2):
        ce = Vcur[b][rig.off_ce:rig.off_ce + rig.me]
        _axpy_close(sce1[b], tce[b], a1[b], ce, "c_e_soc, first round")
        assert np.array_equal(sx[b], p[b][:rig.n]) and np.array_equal(sy[b], -p[b][rig.n:])
    pr.set_params(alpha=np.ones(B), alpha_soc=a2, first=np.zeros(B), active=ACTIVE)
    rig.call(pr.soc_step)
    sce2 = pr.get("sce")
    for b in (0, 2):
        _axpy_close(sce2[b], tce[b], a2[b], sce1[b], "c_e_soc, second round")
    # the right-hand side on its own (the solve that follows it in soc_step may permute the buffer): what
    # eq_soc_rhs_kernel writes is what sqp.hpp:397-468 builds
    rhs = pr.get("sys_rhs")
    for b in (0, 2):
        aty, mag = rig.At(Vcur[b], rig.y[b])
        g = rig.g(Vcur[b])
        top = -g.astype(np.longdouble) + aty
        assert np.all(np.abs(rhs[b][:rig.n] - top) <= 1e-12 * (np.abs(g) + mag) + 1e-300)
        assert np.array_equal(rhs[b][rig.n:], -sce2[b])
    # the trial point along the correction
    alpha = np.array([1.0, 1.0, 0.5])
    pr.set_params(alpha=alpha, mode=np.ones(B), active=ACTIVE)
    rig.call(pr.trial_values, 3)
    tx, ty, sx, sy = (pr.get(k) for k in ("tx", "ty", "sx", "sy"))
    for b in (0, 2):
        _axpy_close(tx[b], rig.x[b], alpha[b], sx[b], "trial x, correction")
        _axpy_close(ty[b], rig.y[b], alpha[b], sy[b], "trial y, correction")


def test_kkt_fallback_and_commit(rig):
    pr = rig.pr
    err = pr.refresh()
    pr.newton_step()
    pr.direction()
    alpha = np.array([1.0, 1.0, 0.5])
    pr.set_params(alpha=alpha, active=ACTIVE)
    ec, et = rig.call(pr.kkt_fallback, len(ebc.ERR_KEYS))
    tx, ty, sysV, sys_in = (pr.get(k) for k in ("tx", "ty", "sys_V", "sys_in"))
    for b in (0, 2):
        assert np.array_equal(ec[b], err[b])  # (the same kernel on the same current point)
        assert np.array_equal(sys_in[b][rig.n:rig.n + rig.me], rig.S[b][1:] * ty[b])
        _check_errors(rig, et[b], sysV[b], tx[b], ty[b], rig.S[b], f"fallback {b}")
    rig.call(pr.commit)
    x, y = pr.get("x"), pr.get("y")
    for b in (0, 2):
        assert np.array_equal(x[b], tx[b]) and np.array_equal(y[b], ty[b])
    assert np.array_equal(x[1], rig.x[1]) and np.array_equal(y[1], rig.y[1])
