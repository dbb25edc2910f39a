"""CPU tier of the dense LDLT edge cases (tests/test_dense_edges_gpu.py is the GPU tier): the host interpreter of the
pivoted dense factorization (hostcheck.cpp: hc_factor_dense_pivoted, hc_solve_dense) against the oracle's dense branch
(oracle/ldlt.hpp: DenseLDLT) on every matrix family of tests/support/dense_models.py at orders 1, 2, 3, 65 and 1025.
This pins the interpreter and the oracle to each other, and shows that the chosen inputs behave as their descriptions
say before a GPU sees them."""
import numpy as np
import pytest

from tests.support import dense_models as dm
from tests.support import model

CPU_ORDERS = (1, 2, 3, 65, 1025)


@pytest.fixture(scope="module")
def interpreters(slpx, hostcheck):
    """HostCheck of the model of an order, compiled once per module."""
    slpx.lib().slpx_graph_reset()
    made = {}

    def get(order):
        if order not in made:
            n, m_e = dm.split(order)
            p = dm.build(model.Model(model.ProductBackend("hostcheck")), n, m_e)
            hc = hostcheck.HostCheck(p.p)
            assert hc.is_dense() and hc.info["ldlt_dense_pivoted"] == 1
            cp, ri = hc.pattern(5)
            ecp, eri = dm.dense_pattern(n, m_e)
            assert np.array_equal(cp, ecp) and np.array_equal(ri, eri)
            made[order] = (hc, (cp, ri))
        return made[order]

    yield get
    for hc, _ in made.values():
        hc.close()


CASES = [(f, o) for f in dm.FAMILIES for o in CPU_ORDERS if dm.defined(f, o)]


@pytest.mark.parametrize("family,order", CASES, ids=[f"{f}-{o}" for f, o in CASES])
def test_host_interpreter_equals_the_oracle(interpreters, family, order):
    """D bit for bit (NaNs in the same places), the four counters and min |D| equal; the solve of an integer rhs bit for
    bit where the arithmetic is exact, within max(4 eta(oracle), dim 2^-53) in backward error otherwise (only where the
    factorization succeeded: a failed one has no solution to be near)."""
    hc, pat = interpreters(order)
    c = dm.case(family, order)
    ref = dm.oracle_factor(family, order)
    hc.set_lhs(dm.values(c.K, pat))
    D, stats = hc.factor(c.delta, c.gamma)
    assert dm.same_bits(D, ref["D"]), np.flatnonzero(~(D == ref["D"]))[:8]
    assert tuple(int(v) for v in stats[:4]) == ref["inertia"] + (ref["n_bad"],), (stats, ref["inertia"], ref["n_bad"])
    assert float(stats[4]) == ref["min_abs"], (stats[4], ref["min_abs"])
    b = dm.integer_rhs(order)
    hc.set_rhs(b)
    p = hc.solve()
    if c.exact:
        assert dm.same_bits(p, ref["x"])
    elif ref["n_bad"] == 0:
        Kreg = dm.regularized(c.K, c.n, c.delta, c.gamma)
        eta, eta_ref = dm.backward_error(Kreg, b, p), dm.backward_error(Kreg, b, ref["x"])
        print(f"{family} order {order}: eta(host) {eta:.3e} eta(oracle) {eta_ref:.3e}")
        assert eta <= dm.solve_bound(eta_ref, order), (eta, eta_ref)


@pytest.mark.parametrize("order", CPU_ORDERS)
def test_the_families_behave_as_described(orc, order):
    """What each family is there for, read off the oracle: ties keep the first index, the zero matrix succeeds, a zero
    diagonal with something beside it fails at once, exact zero pivots after the SPD block and zeros in the solution
    there, a non-zero pivot after a zero one, a pivot below DBL_MIN solved to 0, NaN reported."""
    n, m_e = dm.split(order)
    ident = np.arange(order)
    r = dm.oracle_factor("equal_diagonal", order)
    assert np.array_equal(r["trans"], ident)
    r = dm.oracle_factor("three_level_diagonal", order)
    assert np.all(r["trans"] >= ident)
    if order >= 65:
        assert np.count_nonzero(r["trans"] != ident) > order // 4
    r = dm.oracle_factor("zero", order)
    assert r["info"] == 0 and r["inertia"] == (0, 0, order) and np.array_equal(r["trans"], ident) and not r["x"].any()
    if order >= 2:
        r = dm.oracle_factor("zero_diagonal", order)
        assert r["info"] == 1 and r["n_bad"] == 1
    r = dm.oracle_factor("spd_block_then_zero", order)
    rank = 2 * ((order + 1) // 4)
    assert r["info"] == 0 and r["inertia"] == (rank, 0, order - rank)
    assert np.count_nonzero(r["D"] == 0.0) == order - rank and not r["x"][rank:].any()
    assert rank == 0 or r["x"][:rank].any()
    if order >= 65:
        r = dm.oracle_factor("rank5_integer", order)
        assert r["info"] == 1 and r["D"][0] != 0.0 and (r["D"] == 0.0).any()  # (not the k = 0 exit: found_zero_pivot)
        zero_at = int(np.flatnonzero(r["D"] == 0.0)[0])
        assert (r["D"][zero_at:] != 0.0).any()
    if order >= 3:
        r = dm.oracle_factor("tiny_pivot", order)
        assert r["info"] == 0 and r["D"][-1] == 1e-310 and r["x"][n // 2] == 0.0 and r["min_abs"] == 1e-310
    for name in dm.NAN_FAMILIES:
        r = dm.oracle_factor(name, order)
        assert r["n_bad"] == 1 and np.array_equal(r["trans"], ident)
    r = dm.oracle_factor("quasidefinite", order)
    assert r["info"] == 0 and r["inertia"] == (n, m_e, 0)


def test_the_other_tie_break_changes_D(orc):
    """Eigen's maxCoeff keeps the FIRST of equal |diagonal| entries; the kernel's reduction does so through `oi < bi`
    across lanes and waves.  A restatement of the algorithm in numpy gives the oracle's D bit for bit with the first
    index and another D with the last (what `oi > bi` would choose) on equal_diagonal — on which every step is a tie
    over the whole rest — so the bit-equality of D on that family is a test of the tie-break."""
    for order in (3, 65):
        c = dm.case("equal_diagonal", order)
        ref = dm.oracle_factor("equal_diagonal", order)
        info, D, trans = dm.eigen_ldlt(c.K)
        assert info == ref["info"] and dm.same_bits(D, ref["D"]) and np.array_equal(trans, ref["trans"])
        _, D_last, trans_last = dm.eigen_ldlt(c.K, last_of_equals=True)
        assert not np.array_equal(trans_last, trans)
        if order == 65:  # (three small integers can come out the same either way)
            print("entries of D that differ with the last of equals:", np.count_nonzero(D_last != ref["D"]), "of", order)
            assert not dm.same_bits(D_last, ref["D"])
    c = dm.case("three_level_diagonal", 65)
    ref = dm.oracle_factor("three_level_diagonal", 65)
    info, D, trans = dm.eigen_ldlt(c.K)
    assert info == ref["info"] and dm.same_bits(D, ref["D"]) and np.array_equal(trans, ref["trans"])


@pytest.mark.parametrize("order", CPU_ORDERS)
def test_policy_loop_of_the_oracles_dense_branch(orc, order):
    """The inputs of the GPU tier's compute() tests do what they are for: an indefinite Hessian makes the policy raise
    delta (more than one factorization, a different number for the two shifts), a quasidefinite matrix takes one."""
    n, m_e = dm.split(order)
    one = dm.oracle_compute("quasidefinite", order)
    small, large = dm.oracle_compute("indefinite:5e-4", order), dm.oracle_compute("indefinite:5e-3", order)
    assert one["info"] == small["info"] == large["info"] == 0
    # (below 65 the Hessian G G^T / n - shift I of a handful of variables need not be indefinite, and the model of
    # order 3 — one variable, two constraints — has a rank-deficient Jacobian: its first attempt has a zero pivot)
    if order >= 65:
        assert one["factorizations"] == 1 and one["reg"] == (0.0, 0.0)
        assert small["reg"][0] == 1e-3 and large["reg"][0] == 1e-2
        assert (small["factorizations"], large["factorizations"]) == (3, 4)
