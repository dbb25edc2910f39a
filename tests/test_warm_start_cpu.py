"""CPU tier of warm starts: the formulas of sleipnir_amd/csrc/warm_start.h as the host instantiates them (a stand-alone
program, tests/support/warmcheck_host.cpp, also built with -fsanitize=address,undefined) against the numpy restatement of
tests/support/warmcheck_host.py, and the conventions of the new entry points that need no device.

Bit for bit wherever the formula is single IEEE operations — which is everywhere here: the host does not contract, and
the one sum of the safeguard (the mean of s z) is formed by the caller, not by these functions."""
import ctypes

import numpy as np
import pytest

from tests.support import param_models as pmod
from tests.support import warmcheck_host as wh

C = {k: i for i, k in enumerate(wh.COLUMNS_IN)}
O = {k: i for i, k in enumerate(wh.COLUMNS_OUT)}
NAN, INF = float("nan"), float("inf")


def row(**kw):
    r = dict(v_u=1.0, d_c=1.0, d_f=1.0, mu_given=0.0, sum=0.0, count=0.0, mu_min=1e-9, given_s=1.0, s=1.0, c_i=1.0,
             given_z=1.0, z=1.0)
    r.update(kw)
    return [r[k] for k in wh.COLUMNS_IN]


def table():
    rng = np.random.default_rng(11)
    t = []
    # conversions: scales of 1, and scales as compute_problem_scaling makes them (min(1, 100 / norm): not powers of two)
    for v in (1.0, -3.5, 1e-9, 7e8, 0.0, -0.0, 5e-324, 1.7976931348623157e308):
        t.append(row(v_u=v))
    for _ in range(200):
        t.append(row(v_u=rng.standard_normal() * 10.0 ** rng.integers(-12, 12), d_c=100.0 / rng.uniform(100.0, 1e6),
                     d_f=100.0 / rng.uniform(100.0, 1e6)))
    # non-finite input
    for v in (NAN, INF, -INF):
        t.append(row(v_u=v))
    # mu: given (above and below the floor), chosen from the mean (inside, above the cold value, below the floor), no row
    t.append(row(mu_given=1e-3, d_f=0.25))
    t.append(row(mu_given=1e-12, d_f=0.25, mu_min=2.5e-10))
    t.append(row(sum=3e-4, count=7.0, d_f=0.25, mu_min=2.5e-10))
    t.append(row(sum=30.0, count=7.0, d_f=0.25, mu_min=2.5e-10))
    t.append(row(sum=3e-14, count=7.0, d_f=0.25, mu_min=2.5e-10))
    t.append(row(sum=0.0, count=0.0, d_f=0.25, mu_min=2.5e-10))
    t.append(row(mu_given=-1.0, sum=1e-2, count=1.0))
    # slack: kept, s <= 0 with c_i above and below mu, absent; dual: kept, z <= 0, absent, the clamp on both sides
    for s in (2.0, 1e-9, 0.0, -1.0):
        for c in (3.0, 1e-12, -4.0):
            t.append(row(s=s, c_i=c, mu_given=1e-4))
    t.append(row(given_s=0.0, s=5.0, c_i=0.5, mu_given=1e-4))
    for z in (2.0, 0.0, -1e-3):
        t.append(row(z=z, mu_given=1e-4))
    t.append(row(given_z=0.0, z=5.0, mu_given=1e-4))
    t.append(row(z=1e-16, s=1.0, mu_given=1e-4))   # below mu / (kappa s) = 1e-14
    t.append(row(z=1e7, s=1.0, mu_given=1e-4))     # above kappa mu / s = 1e6
    t.append(row(z=1e-14, s=1.0, mu_given=1e-4))   # on the lower edge: stays
    t.append(row(z=1e-9, s=1e-9, mu_given=1e-9))   # an active row at a solution: kept, no repair
    t.append(row(z=1e-9, s=1.0, mu_given=1e-9))    # an inactive one
    return np.array(t, dtype=np.float64)


def expected(t):
    e = np.zeros((len(t), len(wh.COLUMNS_OUT)))
    for i, a in enumerate(t):
        g = lambda k: a[C[k]]
        with np.errstate(all="ignore"):
            e[i, O["scale_s"]] = wh.scale_s(g("v_u"), g("d_c"))
            e[i, O["unscale_s"]] = wh.unscale_s(e[i, O["scale_s"]], g("d_c"))
            e[i, O["scale_dual"]] = wh.scale_dual(g("v_u"), g("d_c"), g("d_f"))
            e[i, O["unscale_dual"]] = wh.unscale_dual(e[i, O["scale_dual"]], g("d_c"), g("d_f"))
            e[i, O["scale_mu"]] = np.float64(g("d_f")) * np.float64(g("v_u"))
            e[i, O["unscale_mu"]] = e[i, O["scale_mu"]] / np.float64(g("d_f"))
        e[i, O["bad"]] = 0.0 if np.isfinite(g("v_u")) else 1.0
        e[i, O["counts"]] = 1.0 if g("s") > 0.0 and g("z") > 0.0 else 0.0
        mu = wh.choose_mu(g("sum"), g("count"), g("mu_given"), g("d_f"), g("mu_min"))
        e[i, O["mu"]] = mu
        s, rs = wh.slack(g("given_s") != 0.0, g("s"), g("c_i"), mu)
        e[i, O["slack"]], e[i, O["slack_repaired"]] = s, float(rs)
        z, rz = wh.dual(g("given_z") != 0.0, g("z"), mu, s)
        e[i, O["dual"]], e[i, O["dual_repaired"]] = z, float(rz)
    return e


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulps(a, b):
    """distance in units in the last place between finite doubles of one sign"""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.fixture(scope="module")
def results():
    t = table()
    return t, wh.evaluate(t), expected(t)


def test_host_formulas_match_numpy_bit_for_bit(results):
    t, got, want = results
    for k, j in O.items():
        same = (bits(got[:, j]) == bits(want[:, j])) | (np.isnan(got[:, j]) & np.isnan(want[:, j]))
        assert same.all(), (k, t[~same][:3], got[~same, j][:3], want[~same, j][:3])


def test_sanitized_build_gives_the_same_bits(results):
    t, got, _ = results
    san = wh.evaluate(t, sanitized=True)
    assert np.array_equal(bits(san), bits(got))


def test_unit_scales_return_the_bits_and_others_come_back_within_2_ulp(results):
    t, got, _ = results
    finite = np.isfinite(t[:, C["v_u"]])
    unit = finite & (t[:, C["d_c"]] == 1.0) & (t[:, C["d_f"]] == 1.0)
    assert unit.sum() >= 8
    for a, b in (("scale_s", "unscale_s"), ("scale_dual", "unscale_dual"), ("scale_mu", "unscale_mu")):
        assert np.array_equal(bits(got[unit, O[a]]), bits(t[unit, C["v_u"]])), a
        assert np.array_equal(bits(got[unit, O[b]]), bits(t[unit, C["v_u"]])), b
    # (each direction is ONE rounding of the entry — the duals' quotient d_c / d_f is the same double both ways — so
    # out(in(v)) is two roundings from v: at most 2 ulp)
    other = finite & ~unit
    assert other.sum() >= 200
    for b in ("unscale_s", "unscale_dual", "unscale_mu"):
        assert ulps(got[other, O[b]], t[other, C["v_u"]]).max() <= 2, b


def test_the_cases_the_table_is_there_for(results):
    """That the table reaches every branch: s <= 0, z <= 0, absent blocks, NaN, mu given and chosen, both clamp sides."""
    t, got, _ = results
    assert got[:, O["bad"]].sum() == 3
    assert (got[:, O["slack_repaired"]] == 1).sum() >= 7 and (got[:, O["dual_repaired"]] == 1).sum() >= 5
    mu = got[:, O["mu"]]
    lo, hi = mu / (wh.KAPPA * got[:, O["slack"]]), wh.KAPPA * mu / got[:, O["slack"]]
    z_in = t[:, C["z"]]
    given = t[:, C["given_z"]] != 0
    assert (given & (z_in > 0) & (z_in < lo * (1 - 1e-12))).any() and (given & (z_in > hi * (1 + 1e-12))).any()
    # an active and an inactive row of a converged iterate pass untouched
    tail = got[-2:]
    assert np.array_equal(tail[:, O["dual"]], t[-2:, C["z"]]) and not tail[:, O["dual_repaired"]].any()
    assert not tail[:, O["slack_repaired"]].any()


@pytest.fixture
def m(fresh):
    mm = pmod.new_model()
    mm.be.reset()
    return mm


def test_symbols_exist_and_are_declared(slpx):
    L = slpx.lib()
    for name in ("slpx_problem_solve_warm", "slpx_problem_get_iterate", "slpx_problem_solve_batch_warm",
                 "slpx_problem_warm_start_repaired"):
        assert hasattr(L, name) and getattr(L, name).argtypes, name
    header = (wh.ROOT / "include" / "slpx.h").read_text()
    for name in ("slpx_warm_start", "slpx_problem_solve_warm", "slpx_problem_get_iterate", "slpx_problem_solve_batch_warm"):
        assert name in header, name


def test_usage_errors_need_no_device(m, slpx):
    L = slpx.lib()
    pm = pmod.boxed(m, (0.0, 1.0))
    h = pm.p.p._h
    ws = slpx.WarmStart(None, None, None, 0.0)
    assert L.slpx_problem_solve_warm(None, None, 0, ctypes.byref(ws), None) == -100 and b"null problem" in L.slpx_last_error()
    x0 = np.zeros((1, 1))
    args = lambda p, batch: (p, batch, x0.ctypes.data, None, None, None, None, None, None, 0, *([None] * 10), None)
    assert L.slpx_problem_solve_batch_warm(*args(None, 1)) == -100 and b"null problem" in L.slpx_last_error()
    assert L.slpx_problem_solve_batch_warm(*args(h, 0)) == -100 and b"batch must be positive" in L.slpx_last_error()
    pm.p.p.add_callback(lambda info: False)
    assert L.slpx_problem_solve_batch_warm(*args(h, 1)) == -100 and b"callbacks" in L.slpx_last_error()
    pm.p.p.clear_callbacks()
    assert L.slpx_problem_warm_start_repaired(None) == -1
    pm.close()


def test_get_iterate_before_any_solve_is_an_error(m, slpx):
    L = slpx.lib()
    pm = pmod.boxed(m, (0.0, 1.0))
    mu = ctypes.c_double()
    assert L.slpx_problem_get_iterate(None, None, None, None, None, None) == -100 and b"null problem" in L.slpx_last_error()
    assert L.slpx_problem_get_iterate(pm.p.p._h, None, None, None, None, ctypes.addressof(mu)) == -100
    assert b"has not been solved" in L.slpx_last_error()
    with pytest.raises(slpx.SlpxError):
        pm.p.p.iterate()
    pm.close()


def test_python_surface_without_a_device(fresh):
    from sleipnir_amd import optimization

    p = optimization.Problem()
    x = p.decision_variable()
    p.minimize((x - 3) ** 2)
    p.subject_to(x <= 1)
    with pytest.raises(KeyError):
        p.solve(warm_starts=optimization.Iterate())
    with pytest.raises(_SlpxError()):
        p.iterate()
    it = optimization.BatchIterate(s=np.ones((2, 1)), mu=[1e-3, 0.0])
    assert set(it._blocks()) == {"s", "mu"} and optimization.Iterate()._blocks() == {}
    p.close()


def _SlpxError():
    import sleipnir_amd

    return sleipnir_amd.SlpxError
