"""GPU tier: the three kernels of csrc/ldlt_dense_kernels.h at their edges, against the oracle's dense branch
(oracle/ldlt.hpp: DenseLDLT, RegularizedLDLT with use_sparse = false) — tests/test_dense_edges_cpu.py pins the same
inputs on the host first.

All three kernels run 1024 threads over `for (i = tid; i < dim; i += 1024)` loops: order 1025 is the smallest at which a
thread owns two entries (the pivot search's per-thread "first of equals" across two strides included), 1100 puts whole
waves in the second pass; 63 / 64 / 65 and 1023 / 1024 sit either side of a wave and of the workgroup.  The pivoted
kernel's claim is that its D — and so every decision of the regularization policy — is Eigen::LDLT's bit for bit:
asserted on matrices with ties everywhere (equal_diagonal: any tie-break but "the first of equals" changes D, see
test_the_other_tie_break_changes_D of the CPU tier), with Eigen's zero-pivot rules, a pivot below DBL_MIN, and
non-finite input (a NaN matrix used to send the pivot search to row `dim`: into the next instance of a batch)."""
import os

import numpy as np
import pytest

from tests.support import dense_models as dm
from tests.support import model, oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def systems(slpx):
    """System of the model of an order (batch, kernel), compiled once per module.  unpivoted: SLPX_DENSE=1, the plain
    dense kernel on the same model."""
    slpx.lib().slpx_graph_reset()
    made = {}

    def get(order, batch=1, unpivoted=False):
        key = (order, batch, unpivoted)
        if key not in made:
            n, m_e = dm.split(order)
            saved = os.environ.get("SLPX_DENSE")
            if unpivoted:
                os.environ["SLPX_DENSE"] = "1"
            else:
                os.environ.pop("SLPX_DENSE", None)
            try:
                p = dm.build(model.Model(model.ProductBackend("gpu")), n, m_e)
                system = slpx.System(p.p, batch=batch, device=0)
            finally:
                if saved is None:
                    os.environ.pop("SLPX_DENSE", None)
                else:
                    os.environ["SLPX_DENSE"] = saved
            made[key] = (system, system.pattern(5), p)
            assert system.info["ldlt_dense"] == (1 if unpivoted else 2), system.info["ldlt_dense"]
            cp, ri = made[key][1]
            ecp, eri = dm.dense_pattern(n, m_e)
            assert np.array_equal(cp, ecp) and np.array_equal(ri, eri)
        return made[key][:2]

    yield get
    for system, _, p in made.values():
        system.close()
        p.p.close()


def _stats_of(ref):
    return ref["inertia"] + (ref["n_bad"],)


PIVOTED = ([(f, o) for f in dm.EVERY_ORDER_FAMILIES for o in dm.ORDERS] +
           [(f, o) for f in dm.EDGE_FAMILIES for o in dm.EDGE_ORDERS])


@pytest.mark.parametrize("family,order", PIVOTED, ids=[f"{f}-{o}" for f, o in PIVOTED])
def test_pivoted_factor_and_solve(systems, family, order):
    """ldlt_dense_pivoted_factor_kernel, batch 1: D bit-equal to the oracle's, (n_pos, n_neg, n_zero, n_bad) and min |D|
    equal.  ldlt_dense_solve_kernel on those factors: p bit-equal to the oracle's where the arithmetic is exact, else
    eta(device) <= max(4 eta(oracle), dim 2^-53) with eta(p) = |b - K p|_inf / (|K|_inf |p|_inf + |b|_inf), the
    residual in extended precision (only where the factorization succeeded)."""
    system, pat = systems(order)
    c = dm.case(family, order)
    ref = dm.oracle_factor(family, order)
    system.set_lhs(dm.values(c.K, pat)[None, :])
    stats = system.factor(c.delta, c.gamma)[0]
    D = system.get("D")[0]
    assert dm.same_bits(D, ref["D"]), np.flatnonzero(~(D == ref["D"]))[:8]
    assert tuple(int(v) for v in stats[:4]) == _stats_of(ref), (stats, _stats_of(ref))
    assert float(stats[4]) == ref["min_abs"], (stats[4], ref["min_abs"])
    b = dm.integer_rhs(order)
    system.set_rhs(b[None, :])
    system.solve()
    p = system.get("p")[0]
    if c.exact:
        assert dm.same_bits(p, ref["x"])
    elif ref["n_bad"] == 0:
        Kreg = dm.regularized(c.K, c.n, c.delta, c.gamma)
        eta, eta_ref = dm.backward_error(Kreg, b, p), dm.backward_error(Kreg, b, ref["x"])
        print(f"ETA pivoted {family} order {order}: device {eta:.3e} oracle {eta_ref:.3e} bound {dm.solve_bound(eta_ref, order):.3e}")
        assert eta <= dm.solve_bound(eta_ref, order), (eta, eta_ref)


def _compute_alone(system, pat, c, order):
    """compute() + solve() of one matrix on a batch-1 system: (info, (delta, gamma), factorizations, D, p)."""
    system.set_lhs(dm.values(c.K, pat)[None, :])
    system.reset_regularization(1e-10)
    info, reg, nf = system.compute()
    system.set_rhs(dm.integer_rhs(order)[None, :])
    system.solve()
    return int(info[0]), (float(reg[0, 0]), float(reg[0, 1])), nf, system.get("D")[0].copy(), system.get("p")[0].copy()


@pytest.mark.parametrize("order", dm.ORDERS)
def test_pivoted_policy_loop(systems, order):
    """compute() on a matrix whose Hessian is indefinite: the oracle's info, (delta, gamma) and factorization count (one
    less where the product does not launch an attempt its symbolic phase knows to fail), D of the accepted attempt bit
    for bit, the solve within the bound."""
    system, pat = systems(order)
    name = "indefinite:5e-4"
    c = dm.case(name, order)
    ref = dm.oracle_compute(name, order)
    info, reg, nf, D, p = _compute_alone(system, pat, c, order)
    assert info == ref["info"] == 0
    assert reg == ref["reg"], (reg, ref["reg"])
    skipped = 1 if system.info["struct_singular"] and reg[0] != 0.0 else 0
    assert nf + skipped == ref["factorizations"], (nf, skipped, ref["factorizations"])
    assert dm.same_bits(D, ref["D"])
    b = dm.integer_rhs(order)
    Kreg = dm.regularized(c.K, c.n, *reg)
    eta, eta_ref = dm.backward_error(Kreg, b, p), dm.backward_error(Kreg, b, ref["x"])
    print(f"ETA policy {name} order {order}: device {eta:.3e} oracle {eta_ref:.3e} reg {reg} factorizations {nf}")
    assert eta <= dm.solve_bound(eta_ref, order), (eta, eta_ref)


# a different matrix in every slot; the indefinite ones keep the policy loop going after the others have stopped
# (1 attempt for quasidefinite, 3 for the shift 5e-4, 4 for 5e-3 — test_policy_loop_of_the_oracles_dense_branch)
SLOTS = {3: [("quasidefinite", 0), ("indefinite:5e-4", 0), ("quasidefinite", 1)],
         5: [("quasidefinite", 0), ("indefinite:5e-3", 0), ("quasidefinite", 1), ("indefinite:5e-4", 0), ("quasidefinite", 2)]}
_alone = {}


def _alone_cached(systems, name, order, variant):
    key = (name, order, variant)
    if key not in _alone:
        system, pat = systems(order)
        _alone[key] = _compute_alone(system, pat, dm.case(name, order, variant), order)
    return _alone[key]


def _run_batch(systems, order, slots):
    system, pat = systems(order, batch=len(slots))
    system.set_lhs(np.stack([dm.values(dm.case(nm, order, v).K, pat) for nm, v in slots]))
    system.reset_regularization(1e-10)
    info, reg, nf = system.compute()
    system.set_rhs(np.tile(dm.integer_rhs(order), (len(slots), 1)))
    system.solve()
    return info, reg, nf, system.get("D"), system.get("p")


def _assert_slot_equals_alone(systems, order, slot, nm, v, info, reg, D, p):
    a_info, a_reg, _, a_D, a_p = _alone_cached(systems, nm, order, v)
    assert int(info[slot]) == a_info, (slot, nm)
    assert (float(reg[slot, 0]), float(reg[slot, 1])) == a_reg, (slot, nm, reg[slot], a_reg)
    assert dm.same_bits(D[slot], a_D), (slot, nm)
    assert dm.same_bits(p[slot], a_p), (slot, nm)


@pytest.mark.parametrize("order", [65, 1025])
@pytest.mark.parametrize("batch", [3, 5])
def test_batch_slots_equal_their_solo_runs(systems, batch, order):
    """A workgroup per instance, instances that stop at different attempts: every slot's D, p, (delta, gamma) and info
    bit-equal to the same matrix run alone at batch 1; D, (delta, gamma) and info equal to the oracle's (its p is held
    to the solve bound by test_pivoted_policy_loop and here through the solo run: the device's substitution fuses its
    multiply-adds, the oracle's does not, so their bits differ by design)."""
    slots = SLOTS[batch]
    info, reg, nf, D, p = _run_batch(systems, order, slots)
    attempts = []
    for slot, (nm, v) in enumerate(slots):
        _assert_slot_equals_alone(systems, order, slot, nm, v, info, reg, D, p)
        ref = dm.oracle_compute(nm, order, v)
        assert int(info[slot]) == ref["info"] == 0
        assert (float(reg[slot, 0]), float(reg[slot, 1])) == ref["reg"]
        assert dm.same_bits(D[slot], ref["D"])
        c = dm.case(nm, order, v)
        b = dm.integer_rhs(order)
        Kreg = dm.regularized(c.K, c.n, *ref["reg"])
        eta, eta_ref = dm.backward_error(Kreg, b, p[slot]), dm.backward_error(Kreg, b, ref["x"])
        assert eta <= dm.solve_bound(eta_ref, order), (slot, eta, eta_ref)
        attempts.append(ref["factorizations"])
    assert len(set(attempts)) > 1 and nf == max(attempts), (nf, attempts)


@pytest.mark.parametrize("order", [65, 1025])
@pytest.mark.parametrize("batch", [3, 5])
@pytest.mark.parametrize("nan_family", dm.NAN_FAMILIES)
def test_a_nan_instance_leaves_its_neighbours_alone(systems, nan_family, batch, order):
    """What a diverged instance of solve_batch hands the factorization: a NaN matrix in a middle slot (never the last).
    That slot reports info != 0 with the oracle's (delta, gamma); every other slot is bit-equal to its solo run.  Before
    the pivot search followed Eigen's rule on NaN (start at k, move on a strictly greater value only) nothing compared,
    the search answered `dim`, and the transposition k <-> dim exchanged at(0, 0) of the NEXT instance's matrix with an
    entry of this one while that instance was being factored."""
    slots = list(SLOTS[batch])
    middle = batch // 2
    slots[middle] = (nan_family, 0)
    info, reg, nf, D, p = _run_batch(systems, order, slots)
    ref = dm.oracle_compute(nan_family, order)
    assert int(info[middle]) != 0 and ref["info"] != 0
    assert (float(reg[middle, 0]), float(reg[middle, 1])) == ref["reg"], (reg[middle], ref["reg"])
    for slot, (nm, v) in enumerate(slots):
        if slot != middle:
            _assert_slot_equals_alone(systems, order, slot, nm, v, info, reg, D, p)


def _unit_lower(Lx, dim):
    """L of ldlt_dense_factor_kernel's Lx: the strictly lower part column by column, column j at
    j (dim - 1) - j (j - 1) / 2 (LdltPlan::Lp of the dense plan)."""
    L = np.eye(dim)
    cols, rows = np.triu_indices(dim, 1)  # (column, row) of the strictly lower part in column-major order
    assert len(Lx) == len(rows)
    L[rows, cols] = Lx
    return L


def _refined_solution(Kreg, b):
    """The solution of Kreg x = b refined with residuals in extended precision until it moves no more."""
    from tests.support import parity

    dim = len(b)
    cp, ri = dm.dense_pattern(dim, 0)
    val = dm.values(Kreg, (cp, ri))
    x = np.linalg.solve(Kreg, b)
    for _ in range(4):
        x = x + np.linalg.solve(Kreg, parity.residual_longdouble(cp, ri, val, b, x))
    return x


@pytest.mark.parametrize("order", dm.ORDERS)
def test_unpivoted_factor_and_solve(systems, order):
    """ldlt_dense_factor_kernel (SLPX_DENSE=1) on quasidefinite at (0, 1e-10): with L from Lx and D, for every entry
    i >= j, in long double,
        |Kreg - L D L^T|_ij <= gamma_{dim+2} (|L| |D| |L^T|)_ij,   gamma_m = m u / (1 - m u), u = 2^-53.
    Derivation.  The kernel keeps u_jk = a_jk^(k) (unscaled) and l_ik = fl(u_ik fl(1 / d_k)), and updates
    a_ij^(k+1) = fma(-l_ik, u_jk, a_ij^(k)): one rounding per step, j of them before column j is final, so
    a_ij = a_ij^(j) (1 + theta_j) + sum_{k<j} l_ik u_jk (1 + theta_j).  l_jk = u_jk / d_k (1 + theta_2) (the reciprocal
    and the product), so u_jk = l_jk d_k (1 + theta_2), and a_ij^(j) is d_j (i = j) or l_ij d_j (1 + theta_2): every
    term l_ik d_k l_jk, k <= j, carries at most j + 2 <= dim + 1 roundings.  One more unit covers the evaluation of both
    sides here (long double sums of at most 2048 terms: 2048 x 2^-64 = u).  The matrix factored is the kernel's own
    Kreg = fl(K + diag(delta, -gamma)), one addition per diagonal entry.
    The inertia is (n, m_e, 0) by construction; the solve is held to eta <= max(4 eta(refined), dim 2^-53) against a
    solution refined in extended precision."""
    system, pat = systems(order, unpivoted=True)
    c = dm.case("quasidefinite", order)
    dim = order
    system.set_lhs(dm.values(c.K, pat)[None, :])
    stats = system.factor(c.delta, c.gamma)[0]
    assert tuple(int(v) for v in stats[:4]) == (c.n, c.m_e, 0, 0), stats
    D = system.get("D")[0]
    L = _unit_lower(system.get("Lx")[0][:dim * (dim - 1) // 2], dim)
    assert float(stats[4]) == float(np.min(np.abs(D)))
    Kreg = dm.regularized(c.K, c.n, c.delta, c.gamma)
    resid, bound = oracle.ldlt_reconstruction(Kreg, L, D)
    m = dim + 2
    gamma_m = m * U / (1.0 - m * U)
    worst = float(np.max(np.abs(resid) / np.where(bound > 0.0, bound, 1.0)))
    print(f"RECONSTRUCTION unpivoted order {order}: max |Kreg - L D L^T| / (|L||D||L^T|) = {worst:.3e} (gamma_{m} = {gamma_m:.3e})")
    assert np.all(np.abs(resid) <= gamma_m * bound), worst
    b = dm.integer_rhs(order)
    system.set_rhs(b[None, :])
    system.solve()
    p = system.get("p")[0]
    eta, eta_ref = dm.backward_error(Kreg, b, p), dm.backward_error(Kreg, b, _refined_solution(Kreg, b))
    print(f"ETA unpivoted quasidefinite order {order}: device {eta:.3e} refined {eta_ref:.3e} bound {dm.solve_bound(eta_ref, order):.3e}")
    assert eta <= dm.solve_bound(eta_ref, order), (eta, eta_ref)
