"""GPU tier: the kernels of feasibility restoration for a batch (sleipnir_amd/csrc/fr_batch_kernels.h) one launch at a
time, through the probe of BatchFrDevice (tests/support/frbatchcheck.cpp), instance by instance against the high-precision
reference of tests/support/fr_reference.py — the reference, the bounds and the checking code of
tests/test_restoration_kernels_gpu.py, nothing new to measure:
  * lhs, rhs and the direction componentwise, gamma(c + terms) sum|terms| with C_LHS, C_RHS, C_EXPAND;
  * sums within (len + 4) 2^-53 sum|terms| (fr_reference._sum_with_bound).

Shapes: B = 3 on tiny, ineq_only, eq_only (the dense plan; m_e = 0 and m_i = 0 included) and on chain300 (pair lists), B = 64
on chain300 (the batch-interleaved factorization).  Slot k of a batch holds the state KINDS[k % 3]: a mild state, a stiff one
(rows with Sigma = 1e21 and 1e-21), and a slot that is masked out — each kind with its own delta, mu, tau, step sizes and
scales, the masked one with NaN for all of them.  Slots of one kind hold the same state, so at B = 64 the reference is
computed for two instances and every other instance is compared with its twin, bit for bit.

One pass through all kernels (`run_pass`) records every output of every instance; it is made once per arrangement of the
states over the slots and per mask, and the tests read the recordings:
  * every kernel against the reference (`test_*_against_the_reference`);
  * the masked slot untouched, bit for bit, in every buffer of the device struct and in its slices of lhs / rhs;
  * an instance's outputs bit-identical at any slot, under any mask of the others, and run twice;
  * the built systems factor and solve on the plan of the shape (residual of the batch system's own double-double check);
  * a REPORT (printed, not asserted) of whether the row-local outputs have the single-problem kernels' bits.
"""
import copy

import numpy as np
import pytest

from tests.support import fr_models, fr_reference as ref, frbatchcheck, model
from tests.test_restoration_kernels_gpu import (LD, SEED, U, check_errors, check_expansion, lhs_reference, same_bits,
                                                updated_reference, within)

pytestmark = pytest.mark.gpu

SHAPES = [("tiny", 3), ("ineq_only", 3), ("eq_only", 3), ("chain300", 3), ("chain300", 64)]
KINDS = ["mild", "stiff", "masked"]
# per kind: delta, mu, tau, the second trial step (x alpha_max), the commit's step (x alpha_max) and alpha_z
PARAMS = {"mild": dict(delta=1e-4, mu=0.1, tau=0.99, trial=0.3, step=0.5, alpha_z=0.7, mu_outer=0.1),
          "stiff": dict(delta=4e-4, mu=0.05, tau=0.995, trial=0.6, step=0.25, alpha_z=0.4, mu_outer=0.02),
          "masked": dict(delta=np.nan, mu=np.nan, tau=np.nan, trial=np.nan, step=np.nan, alpha_z=np.nan, mu_outer=np.nan)}
A_SOC2 = 0.5  # the second accumulation's alpha


class Rig:
    """One compiled model at one batch size: problem, batch system, probe, the states of the three kinds."""

    def __init__(self, sa, name, B):
        from tests.support import frbatchcheck

        self.name, self.B = name, B
        problem, self.start = fr_models.make(model.Model(model.ProductBackend("gpu")), name)
        self.handle = problem.p
        self.system = sa.System(self.handle, batch=B, device=0)
        self.probe = frbatchcheck.BatchFrProbe(self.system)
        pr = self.probe
        self.n, self.me, self.mi, self.M, self.dim = pr.n, pr.m_e, pr.m_i, pr.M, pr.dim
        self.info = self.system.info
        self.lhs_pattern = self.system.pattern(5)
        self.states = {"mild": ref.random_state(self.start, self.n, self.me, self.mi, SEED, False),
                       "stiff": ref.random_state(self.start, self.n, self.me, self.mi, SEED, True),
                       "masked": ref.random_state(self.start, self.n, self.me, self.mi, SEED + 7, False)}
        rng = np.random.default_rng(SEED + 1)
        self.p = {k: rng.uniform(-1, 1, self.dim) for k in KINDS}
        self.p_soc = {k: 0.5 * v + 0.01 for k, v in self.p.items()}
        self.passes = {}
        self.refs = {}

    def close(self):
        self.probe.close()
        self.system.close()
        self.handle.close()


@pytest.fixture(scope="module")
def rigs(slpx):
    slpx.lib().slpx_graph_reset()
    made = {}

    def get(name, B):
        if (name, B) not in made:
            made[(name, B)] = Rig(slpx, name, B)
        return made[(name, B)]

    yield get
    for r in made.values():
        r.close()
    slpx.lib().slpx_graph_reset()


def kinds_of(B, shift=0):
    return [KINDS[(k + shift) % 3] for k in range(B)]


def run_pass(r, kinds, active):
    """Every kernel once, in the order of an iteration with one second-order correction; returns the recordings:
    rec[stage][buffer or scalars] = array [B][...]."""
    pr, B = r.probe, r.B
    own = list(frbatchcheck.OWN)
    per = lambda key: np.array([PARAMS[k][key] for k in kinds])
    rec = {}

    def snap(stage, extra=(), scalars=None):
        rec[stage] = {q: pr.get(q) for q in own + list(extra)}
        if scalars is not None:
            rec[stage]["scalars"] = scalars

    scales = np.ones((B, pr.ns))
    for b, k in enumerate(kinds):
        st = r.states[k]
        pr.begin(b, st)
        scales[b, 1:] = st["scales"][1:]
    pr.set_scales(scales)
    # (what a skipped instance must keep: recognizable values in the buffers no begin() fills)
    for q in own:
        if q not in ("x", "s0", "y", "z0", "xr", "w", "g_outer", "s_outer", "pn", "sx", "zx"):
            width = pr.get(q).shape[1]
            pr.put(q, np.tile(1000.0 + np.arange(width, dtype=float), B))  # (the same in every slot: slots are compared)
    pr.put("sys_lhs", np.tile(-7.0 - np.arange(pr.nnz_lhs, dtype=float), B))
    pr.put("sys_rhs", np.tile(-9.0 - np.arange(pr.dim, dtype=float), B))
    pr.set_params(delta=per("delta"), mu=per("mu"), tau=per("tau"), alpha=0.0, alpha_soc=0.0, alpha_z=per("alpha_z"),
                  mu_outer=per("mu_outer"), soc=0, first=0, rhs_only=0, active=np.asarray(active, dtype=np.uint8))
    snap("begin", extra=("sys_lhs", "sys_rhs"))
    pr.sweep()
    snap("sweep")
    pr.build()
    snap("build", extra=("sys_lhs", "sys_rhs"))
    # the built systems on the plan of this shape: factor (delta added there, gamma = 0) and solve, the system's own residual
    d = np.where(np.asarray(active) != 0, np.nan_to_num(per("delta")), 1.0)
    r.system.factor(d, np.zeros(B))
    r.system.solve()
    res, norm = r.system.residual(mask=np.asarray(active, dtype=np.uint8))
    rec["factor"] = dict(norm=norm, p=r.system.get("p"))
    pr.put("sys_p", np.array([r.p[k] for k in kinds]))
    dirs = pr.expand()
    snap("expand", extra=("sys_in",), scalars=dirs)
    pr.save_direction()
    snap("save")
    amax = np.array([d_["alpha_max"] for d_ in dirs])
    pr.set_params(alpha=amax)
    met = pr.trial_values(after_expand=True)
    snap("trial_full", extra=("sys_in", "sys_V"), scalars=met)
    pr.set_params(alpha_soc=amax, first=1)
    pr.soc_accumulate()
    snap("soc1")
    pr.set_params(alpha_soc=A_SOC2, first=0)
    pr.soc_accumulate()
    snap("soc2")
    pr.set_params(soc=1, rhs_only=1)
    pr.build()
    snap("soc_build", extra=("sys_lhs", "sys_rhs"))
    pr.put("sys_p", np.array([r.p_soc[k] for k in kinds]))
    sdirs = pr.expand()
    snap("soc_expand", extra=("sys_in",), scalars=sdirs)
    pr.restore_direction()
    snap("restore")
    pr.set_params(soc=0, rhs_only=0, alpha=np.nan_to_num(per("trial")) * amax)
    met2 = pr.trial_values()
    snap("trial_short", extra=("sys_in", "sys_V"), scalars=met2)
    pr.set_params(alpha=np.nan_to_num(per("step")) * amax)
    pr.commit()
    snap("commit")
    pr.sweep()
    errs = pr.errors(True)
    snap("errors", scalars=errs)
    return rec


def the_pass(r, shift=0, mask="all"):
    """cached: the states shifted by `shift` slots; mask "all": every slot but the masked kind's, "one": the first stiff slot alone"""
    key = (shift, mask)
    if key not in r.passes:
        kinds = kinds_of(r.B, shift)
        if mask == "all":
            active = [k != "masked" for k in kinds]
        else:
            active = [b == kinds.index("stiff") for b in range(r.B)]
        r.passes[key] = (kinds, active, run_pass(r, kinds, active))
    return r.passes[key]


def problem_at(r, rec, stage, b, kind, iterate=None):
    """the reference's view of instance b from the device's own current V of that stage"""
    st = {k: v for k, v in r.states[kind].items()}
    if iterate is not None:
        st.update(iterate)
    return ref.problem_from_V(r.info, r.system.pattern, rec[stage]["Vcur"][b], st)


def slot_of(kinds, kind):
    return kinds.index(kind)


def direction_of(r, rec, stage, b):
    s = rec[stage]
    d = s["scalars"][b]
    return dict(dpn=s["dpn"][b], psx=s["psx"][b], pzx=s["pzx"][b], ps0=s["ps0"][b], pz0=s["pz0"][b], dir=d,
                trial_x=s["sys_in"][b][:r.n], alpha=np.array([d[q] for q in ("alpha_max", "alpha_z", "D_phi", "eliminated_min_pivot")]))


# ---------------------------------------------------------------------------------------------------------------------
# every kernel against the reference, per instance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mild", "stiff"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_build_against_the_reference(rigs, name, B, kind):
    """lhs and rhs of the instance with its own delta and mu, componentwise (C_LHS, C_RHS)."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    b = slot_of(kinds, kind)
    P = problem_at(r, rec, "sweep", b, kind)
    r.refs[("P", kind)] = P
    prm = PARAMS[kind]
    want, bound, rwant, rbound = lhs_reference(r, P, prm["mu"], prm["delta"])
    print(f"{name} B={B} {kind} (slot {b}): {r.probe.nnz_lhs} entries")
    within("lhs", rec["build"]["sys_lhs"][b], want, bound)
    within("rhs", rec["build"]["sys_rhs"][b], rwant, rbound)


@pytest.mark.parametrize("name,B", SHAPES)
def test_built_systems_factor_and_solve(rigs, name, B):
    """The systems build() wrote go the way a caller-written system goes (pair lists, il_gather_kernel at B = 64, the
    dense plan): after factor(delta[b], 0) and solve(), the batch system's own double-double residual r = rhs - Kreg p of
    every active instance is a normwise backward error of rounding size,
        max|r| <= 1e3 dim 2^-53 (max|rhs| + ||Kreg||_1 max|p|):
    dim 2^-53 is the bound of a backward-stable LDL^T per unit of element growth, 1e3 the allowance for that growth
    (unpivoted, quasi-definite); the check is on the ROUTE — a system gathered wrongly leaves r of the size of rhs, thirteen
    orders above."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    colptr, rowidx = r.lhs_pattern
    cols = np.repeat(np.arange(r.dim), np.diff(colptr))
    off = rowidx != cols
    for b in range(B):
        if not active[b]:
            continue
        a = np.abs(rec["build"]["sys_lhs"][b])
        col_sums = np.zeros(r.dim)
        np.add.at(col_sums, cols, a)
        np.add.at(col_sums, rowidx[off], a[off])
        col_sums[:r.n] += PARAMS[kinds[b]]["delta"]
        k1 = float(col_sums.max())
        rhs_inf, p_inf = float(np.max(np.abs(rec["build"]["sys_rhs"][b]))), float(np.max(np.abs(rec["factor"]["p"][b])))
        bound = 1e3 * r.dim * U * (rhs_inf + k1 * p_inf)
        norm = rec["factor"]["norm"][b]
        if b < 2:
            print(f"{name} B={B} slot {b}: max|r| {norm:.3g}, bound {bound:.3g} (||K||_1 {k1:.3g}, max|p| {p_inf:.3g}, max|rhs| {rhs_inf:.3g})")
        assert np.isfinite(norm) and norm <= bound, (b, norm, bound)


@pytest.mark.parametrize("kind", ["mild", "stiff"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_expand_against_the_reference(rigs, name, B, kind):
    """The whole direction from p, the step sizes exactly, D_phi, the smallest eliminated pivot and the first trial x
    (check_expansion of the single-problem test: C_EXPAND)."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    b = slot_of(kinds, kind)
    P = problem_at(r, rec, "sweep", b, kind)
    prm = PARAMS[kind]
    E = ref.expand_exact(P, r.p[kind], prm["mu"], prm["delta"], prm["tau"])
    E["delta"] = prm["delta"]
    D = direction_of(r, rec, "expand", b)
    assert same_bits(rec["expand"]["p"][b], r.p[kind])  # the system's solution, kept
    check_expansion(r, P, D, E, r.p[kind], prm["mu"], prm["tau"])


def trial_reference(r, P, D, alpha, trial_x, Vt):
    Pt = copy.copy(P)
    Pt.x = trial_x
    pn = np.asarray(P.pn, LD) + LD(alpha) * np.asarray(D["dpn"], LD)
    S = np.concatenate([np.asarray(P.s0, LD) + LD(alpha) * np.asarray(D["ps0"], LD), np.asarray(P.sx, LD) + LD(alpha) * np.asarray(D["psx"], LD)])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = ref.filter_entry(Pt, pn, S, Vt[1:1 + r.me], Vt[1 + r.me:1 + r.me + r.mi])
        e_pn = 2 * U * (np.abs(P.pn) + np.abs(alpha * D["dpn"]))
        e_S = 2 * U * (np.concatenate([np.abs(P.s0), np.abs(P.sx)]) + np.abs(alpha) * np.concatenate([np.abs(D["ps0"]), np.abs(D["psx"])]))
        extra = {"f": ref.RHO * float(e_pn.sum()), "viol": float(3 * e_pn.sum() + e_S.sum()), "logsum": float(np.sum(e_S / np.abs(S)))}
    return want, extra


@pytest.mark.parametrize("stage", ["trial_full", "trial_short"])
@pytest.mark.parametrize("kind", ["mild", "stiff"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_trial_metrics_against_the_reference(rigs, name, B, kind, stage):
    """f, violation and sum ln s at X + alpha dX after a value sweep: at alpha_max (the trial x expand left) and at the
    instance's own shorter step (trial_point); sums within their bound."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    b = slot_of(kinds, kind)
    P = problem_at(r, rec, "sweep", b, kind)
    D = direction_of(r, rec, "expand", b)
    a = D["dir"]["alpha_max"] * (1.0 if stage == "trial_full" else PARAMS[kind]["trial"])
    trial_x = rec[stage]["sys_in"][b][:r.n]
    within("trial x", trial_x, np.asarray(P.x, LD) + LD(a) * np.asarray(r.p[kind][:r.n], LD), 2 * U * (np.abs(P.x) + np.abs(a * r.p[kind][:r.n])))
    got = rec[stage]["scalars"][b]
    want, extra = trial_reference(r, P, D, a, trial_x, rec[stage]["sys_V"][b])
    print(f"{name} B={B} {kind} {stage} alpha={a!r}: {got}")
    for q in ("f", "viol", "logsum"):
        v, bnd = want[q]
        if np.isnan(float(v)):
            assert np.isnan(got[q]), q
        else:
            within(q, [got[q]], [v], [bnd + extra[q]])
    assert got["finite"] == 1.0


@pytest.mark.parametrize("kind", ["mild", "stiff"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_second_order_correction_against_the_reference(rigs, name, B, kind):
    """soc_accumulate(first) and a second accumulation (8 2^-53 sum|terms|), the corrected right-hand side with the lhs
    left alone, and the corrected direction from the device's accumulators — the single-problem test's checks."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    b = slot_of(kinds, kind)
    P = problem_at(r, rec, "sweep", b, kind)
    prm = PARAMS[kind]
    D = direction_of(r, rec, "expand", b)
    me, mi = r.me, r.mi
    a1 = D["dir"]["alpha_max"]
    Vt = rec["trial_full"]["sys_V"][b]
    ce_t, ci_t = np.asarray(Vt[1:1 + me], LD), np.asarray(Vt[1 + me:1 + me + mi], LD)
    pn, dpn = np.asarray(P.pn, LD), np.asarray(D["dpn"], LD)
    sx, psx, s0, ps0 = np.asarray(P.sx, LD), np.asarray(D["psx"], LD), np.asarray(P.s0, LD), np.asarray(D["ps0"], LD)
    split = lambda v: (v[:me], v[me:2 * me], v[2 * me:2 * me + mi], v[2 * me + mi:])

    def accumulate(alpha, prev, prev_mag):
        al = LD(alpha)
        pnt = pn + al * dpn
        pe, ne, pi, ni = split(pnt)
        mag_pn = np.abs(pn) + np.abs(al * dpn)
        mpe, mne, mpi, mni = split(mag_pn)
        t_ce = ce_t - pe + ne
        t_c0 = (ci_t - pi + ni) - (s0 + al * ps0)
        t_x = pnt - (sx + al * psx)
        m_ce = np.abs(ce_t) + mpe + mne
        m_c0 = np.abs(ci_t) + mpi + mni + np.abs(s0) + np.abs(al * ps0)
        m_x = mag_pn + np.abs(sx) + np.abs(al * psx)
        return [al * pv + t for pv, t in zip(prev, (t_ce, t_c0, t_x))], [abs(alpha) * pm + m for pm, m in zip(prev_mag, (m_ce, m_c0, m_x))]

    pe, ne, pi, ni = split(pn)
    first = [np.asarray(P.ce, LD) - pe + ne, (np.asarray(P.ci, LD) - pi + ni) - s0, pn - sx]
    first_mag = [np.abs(np.asarray(P.ce, LD)) + pe + ne, np.abs(np.asarray(P.ci, LD)) + pi + ni + s0, pn + sx]
    want, mag = accumulate(a1, first, first_mag)
    names = ("soc_ce", "soc_c0", "soc_x")
    for q, w_, m_ in zip(names, want, mag):
        within(q + " (first)", rec["soc1"][q][b], w_, 8 * U * m_)
    got1 = [rec["soc1"][q][b] for q in names]
    want2, mag2 = accumulate(A_SOC2, [np.asarray(g, LD) for g in got1], [np.abs(g) for g in got1])
    for q, w_, m_ in zip(names, want2, mag2):
        within(q + " (second)", rec["soc2"][q][b], w_, 8 * U * m_)
    Ps = copy.copy(P)
    Ps.soc_ce, Ps.soc_c0, Ps.soc_x = (rec["soc2"][q][b] for q in names)
    _, _, rwant, rbound = lhs_reference(r, Ps, prm["mu"], prm["delta"], soc=True)
    within("soc rhs", rec["soc_build"]["sys_rhs"][b], rwant, rbound)
    assert same_bits(rec["soc_build"]["sys_lhs"][b], rec["build"]["sys_lhs"][b])  # rhs_only
    E = ref.expand_exact(Ps, r.p_soc[kind], prm["mu"], prm["delta"], prm["tau"], soc=True)
    E["delta"] = prm["delta"]
    check_expansion(r, Ps, direction_of(r, rec, "soc_expand", b), E, r.p_soc[kind], prm["mu"], prm["tau"])


@pytest.mark.parametrize("name,B", SHAPES)
def test_save_and_restore_direction(rigs, name, B):
    """save_direction keeps the Newton direction's bits, the corrected expand overwrites the direction, restore_direction
    brings the same bits back — per active instance."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    pairs = (("p", "keep_p"), ("ps0", "keep_ps0"), ("pz0", "keep_pz0"), ("dpn", "keep_dpn"), ("psx", "keep_psx"), ("pzx", "keep_pzx"))
    for b in range(B):
        if not active[b]:
            continue
        for q, kept in pairs:
            assert same_bits(rec["save"][kept][b], rec["expand"][q][b]), (b, kept)
            assert same_bits(rec["restore"][q][b], rec["expand"][q][b]), (b, q)
        assert not same_bits(rec["soc_expand"]["p"][b], rec["expand"]["p"][b])
        assert r.M == 0 or not same_bits(rec["soc_expand"]["dpn"][b], rec["expand"]["dpn"][b])


@pytest.mark.parametrize("kind", ["mild", "stiff"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_commit_against_the_reference(rigs, name, B, kind):
    """interior_point.hpp:775-801 on the instance's whole iterate with ITS alpha, alpha_z and mu: x, y, s_0, p / n and their
    slacks within two roundings, the duals reset into [mu / (kappa s), kappa mu / s] of the new slack."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    b = slot_of(kinds, kind)
    P = problem_at(r, rec, "sweep", b, kind)
    prm = PARAMS[kind]
    D = direction_of(r, rec, "expand", b)
    p = r.p[kind]
    a, az, mu = prm["step"] * D["dir"]["alpha_max"], prm["alpha_z"], prm["mu"]
    Bv = {q: rec["commit"][q][b] for q in ("x", "y", "s0", "z0", "pn", "sx", "zx")}
    W = updated_reference(r, P, D, p, a, az, mu)
    within("x", Bv["x"], *W["x"])
    within("y", Bv["y"], *W["y"])
    within("s_0", Bv["s0"], *W["s"])
    within("pn", Bv["pn"], *W["pn"])
    within("sx", Bv["sx"], *W["sx"])
    for what, z, pz, s_new, got in (("z_0", P.z0, D["pz0"], Bv["s0"], Bv["z0"]), ("zx", P.zx, D["pzx"], Bv["sx"], Bv["zx"])):
        zn = np.asarray(z, LD) + LD(az) * np.asarray(pz, LD)
        bound = 2 * U * (np.abs(z) + np.abs(az * pz))
        lo, hi = LD(1.0) / LD(ref.KAPPA) * LD(mu) / np.asarray(s_new, LD), LD(ref.KAPPA) * LD(mu) / np.asarray(s_new, LD)
        want = np.where(zn < lo, lo, np.where(zn > hi, hi, zn))
        within(what, got, want, np.maximum(bound, 4 * U * np.abs(want)))


@pytest.mark.parametrize("kind", ["mild", "stiff"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_errors_against_the_reference(rigs, name, B, kind):
    """All 29 numbers of FrErrOut at the committed, freshly swept iterate, with the instance's scales and mu_outer: the
    restoration problem's reductions, the OUTER problem's f, violation, sum ln s and D_phi from the point of entry, and the
    unregularized eliminated minimum pivot (fr_reference.error_norms, check_errors of the single-problem test)."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    b = slot_of(kinds, kind)
    it = {q: rec["commit"][q][b] for q in ("x", "y", "s0", "z0", "pn", "sx", "zx")}
    st = dict(it)
    st["mu_outer"] = PARAMS[kind]["mu_outer"]
    P = problem_at(r, rec, "errors", b, kind, iterate=st)
    got = rec["errors"]["scalars"][b]
    check_errors(name, got, ref.error_norms(P))


# ---------------------------------------------------------------------------------------------------------------------
# masking and determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", SHAPES)
def test_a_masked_slot_is_untouched(rigs, name, B):
    """Every buffer of the device struct, and lhs / rhs of the batch system, keep the bits they had before the first launch
    in the slices of every instance whose active flag is 0 — after every kernel of the pass."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    masked = [b for b in range(B) if not active[b]]
    assert masked and len(masked) < B
    for stage, s in rec.items():
        if stage in ("begin", "factor"):
            continue
        for q, v in s.items():
            if q in ("scalars", "sys_in", "sys_V"):  # (the shared tape input and V are scratch: a sweep covers every instance)
                continue
            for b in masked:
                assert same_bits(v[b], rec["begin"][q][b]), (stage, q, b)
    # ... and with one instance alone active, everybody else
    kinds1, active1, rec1 = the_pass(r, mask="one")
    for stage, s in rec1.items():
        if stage in ("begin", "factor"):
            continue
        for q, v in s.items():
            if q in ("scalars", "sys_in", "sys_V"):
                continue
            for b in range(B):
                if not active1[b]:
                    assert same_bits(v[b], rec1["begin"][q][b]), (stage, q, b)


def outputs_of(rec, b):
    """everything the pass recorded of instance b, as (stage, name, array) with the scalars as arrays"""
    for stage, s in rec.items():
        if stage in ("begin", "factor"):
            continue
        for q, v in s.items():
            if q == "scalars":
                yield stage, q, np.array(list(v[b].values()))
            elif q not in ("sys_in", "sys_V"):
                yield stage, q, v[b]


@pytest.mark.parametrize("name,B", SHAPES)
def test_an_instance_does_not_depend_on_its_slot_or_on_the_others(rigs, name, B):
    """The outputs of an instance are bit-identical (a) in every slot that holds the same state (B = 64: 21 twins a kind),
    (b) with the states moved on by one and by two slots, (c) with every other instance masked out, (d) run twice."""
    r = rigs(name, B)
    kinds, active, rec = the_pass(r)
    first = {k: kinds.index(k) for k in ("mild", "stiff")}
    base = {k: list(outputs_of(rec, first[k])) for k in first}
    compared = 0
    for b in range(B):  # (a)
        if active[b] and b != first[kinds[b]]:
            for (stage, q, v), (_, _, w) in zip(outputs_of(rec, b), base[kinds[b]]):
                assert same_bits(v, w), ("twin", b, stage, q)
            compared += 1
    assert compared == sum(active) - 2
    for shift in (1, 2):  # (b)
        kinds_s, active_s, rec_s = the_pass(r, shift=shift)
        for k in first:
            b = kinds_s.index(k)
            assert b != first[k]
            for (stage, q, v), (_, _, w) in zip(outputs_of(rec_s, b), base[k]):
                assert same_bits(v, w), ("shift", shift, k, stage, q)
    kinds1, active1, rec1 = the_pass(r, mask="one")  # (c)
    b = kinds1.index("stiff")
    for (stage, q, v), (_, _, w) in zip(outputs_of(rec1, b), base["stiff"]):
        assert same_bits(v, w), ("alone", stage, q)
    again = run_pass(r, kinds, active)  # (d)
    for k in first:
        for (stage, q, v), (_, _, w) in zip(outputs_of(again, first[k]), base[k]):
            assert same_bits(v, w), ("twice", k, stage, q)


# ---------------------------------------------------------------------------------------------------------------------
# report: the single-problem kernels' bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "ineq_only", "eq_only", "chain300"])
def test_report_bits_against_the_single_kernels(rigs, slpx, name):
    """REPORT, not a requirement: do the row-local outputs — lhs, rhs, dpn, psx, pzx, ps0, pz0 — of the batched kernels have
    the bits of fr_build_kernel / fr_expand_kernel (through frcheck) on the same V, state, p, delta and mu?  The row bodies
    are one source (fr_rows.h) and the loops are the same; the compiler is free to contract differently in two kernels."""
    from tests.support import frcheck

    r = rigs(name, 3)
    kinds, active, rec = the_pass(r)
    problem, _ = fr_models.make(model.Model(model.ProductBackend("gpu")), name)
    single = slpx.System(problem.p, batch=1, device=0)
    fp = frcheck.FrProbe(single)
    try:
        for kind in ("mild", "stiff"):
            b = kinds.index(kind)
            st, prm = r.states[kind], PARAMS[kind]
            fp.set_outer(st["x"], st["s0"], st["y"], st["z0"])
            fp.begin(st["xr"], st["w"], st["g_outer"], st["s_outer"], st["mu_outer"], st["pn"], st["sx"], st["zx"], st["scales"])
            fp.put("V", rec["sweep"]["Vcur"][b])
            fp.build(prm["delta"], prm["mu"])
            fp.put("p", r.p[kind])
            fp.expand(prm["delta"], prm["mu"], prm["tau"])
            dpn, psx, pzx = fp.download_direction()
            single_out = dict(lhs=fp.get("lhs_raw"), rhs=fp.get("rhs_raw"), dpn=dpn, psx=psx, pzx=pzx, ps0=fp.get("p_s"), pz0=fp.get("p_z"))
            batch_out = dict(lhs=rec["build"]["sys_lhs"][b], rhs=rec["build"]["sys_rhs"][b], **{q: rec["expand"][q][b] for q in ("dpn", "psx", "pzx", "ps0", "pz0")})
            verdict = {q: bool(same_bits(np.asarray(single_out[q]), np.asarray(batch_out[q]))) for q in single_out}
            print(f"REPORT {name} {kind}: same bits as the single kernels: {verdict}")
            for q in single_out:
                assert np.asarray(single_out[q]).shape == np.asarray(batch_out[q]).shape, q
    finally:
        fp.close()
        single.close()
        problem.p.close()
