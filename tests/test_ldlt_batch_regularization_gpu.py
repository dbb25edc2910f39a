"""GPU tier: the batched LDL^T when the instances of ONE batch end on DIFFERENT rungs of the regularization ladder.

NewtonSystem::compute_impl -> ldlt_run_batch -> DeviceNlp::factor makes one launch per rung; an instance that is
already accepted stays in the batch with delta = NaN, and every factorization kernel has to leave its L, D, z, update
blocks and solution as its own accepted attempt left them while the other lanes of the same wave or group go on to
larger delta.  The matrices (tests/support/reg_models.py) are built so that the reference's policy restated on
eigenvalues — expected(), numpy alone — decides every expected value: eight classes on one pattern that accept at
(0, 0), 1e-4, 1e-4, 1e-3, 1e-1, 1, 100 and never (tests/test_reg_models_cpu.py asserts the margins of those decisions).

Paths: the per-task kernels in one launch and in a launch per round, the interleaved kernels with one partly filled
group of 16 and with 64 + 6 instances, the per-task kernels at 70, the two dense kernels.  Per path:
decisions, linear algebra per instance against numpy, a masked lane's bits against a batch where nothing is masked,
a permutation of the batch, the per-instance memory over three compute() calls, and the mask one launch at a time.

L, D, z and the update blocks are read back per instance (slpx_system_get 6, 7, 12, 13): the update blocks are read by
nobody but the next round of the same attempt, so a masked lane that overwrites them changes no solution — and still
breaks the rule every later reader of those buffers may rely on.

Not here: the same seam under a Newton step (mode 1: every attempt followed at once by the solve, which writes p for
the whole batch).  A test of it — batches of 6 and 70 cart-pole N = 8 states, every third at the state of
golden/cart_pole_N8_indefinite.npz — ended in a segmentation fault inside slpx_system_create of the batch of six, on
the host, before any of its launches; the cause was not found, so that test is not part of this file."""
import contextlib
import os

import numpy as np
import pytest

from tests.support import cases
from tests.support import reg_models as rm

pytestmark = pytest.mark.gpu

SWITCHES = ("SLPX_SINGLE_LAUNCH", "SLPX_IL_MIN_BATCH", "SLPX_LDLT_IL", "SLPX_DENSE", "SLPX_TASK_ENTRIES", "SLPX_LDLT_MF")
# path -> batch, the switches it is made under, the model; what must be true of the system made
PATHS = {
    "tasks-one-launch": dict(B=5, env={}, shape="sparse", interleaved=False, single_launch=True),
    "tasks-launch-per-round": dict(B=5, env={"SLPX_SINGLE_LAUNCH": "0"}, shape="sparse", interleaved=False, single_launch=False),
    "interleaved-5": dict(B=5, env={"SLPX_IL_MIN_BATCH": "1"}, shape="sparse", interleaved=True),
    "interleaved-70": dict(B=70, env={}, shape="sparse", interleaved=True),
    "tasks-70": dict(B=70, env={"SLPX_LDLT_IL": "0"}, shape="sparse", interleaved=False),
    "dense-plain": dict(B=5, env={"SLPX_DENSE": "1"}, shape="dense", dense=1),
    "dense-pivoted": dict(B=5, env={}, shape="dense", dense=2),
}
PATH_IDS = list(PATHS)
FACTOR_OUTPUTS = ("Lx", "D", "zv", "update_blocks")


@contextlib.contextmanager
def _switches(env):
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _interleaved_rule(B):
    """interleaved_for (csrc/system_choice.hpp), from the switches it honours."""
    if os.environ.get("SLPX_LDLT_IL", "1")[0] == "0":
        return False
    return B >= int(os.environ.get("SLPX_IL_MIN_BATCH", "64"))


class Seam:
    """One system of a path: the linear-solver handle (or, for the pivoted dense kernel, which only a compiled model
    reaches, the model of tests/support/dense_models.py with the matrices installed by set_lhs)."""

    def __init__(self, slpx, path):
        spec = PATHS[path]
        self.path, self.B, self.shape = path, spec["B"], spec["shape"]
        self.m = rm.model(self.shape)
        self.problem = None
        m = self.m
        with _switches(spec["env"]):
            if spec.get("dense") == 2:
                from tests.support import dense_models as dm
                from tests.support import model

                slpx.lib().slpx_graph_reset()
                self.problem = dm.build(model.Model(model.ProductBackend("gpu")), m.n, m.m_e)
                self.ls = slpx.System(self.problem.p, batch=self.B, device=0)
                cp, ri = self.ls.pattern(5)
                assert np.array_equal(cp, m.colptr) and np.array_equal(ri, m.rowidx)
                self.set_matrix = self.ls.set_lhs
            else:
                self.ls = slpx.System.linear_solver(m.n, m.m_e, m.colptr, m.rowidx, batch=self.B)
                self.set_matrix = self.ls.set_matrix
            info = self.ls.info
            # the path that was meant is the path that runs
            assert info["ldlt_dense"] == spec.get("dense", 0), (path, info["ldlt_dense"])
            if not spec.get("dense"):
                assert _interleaved_rule(self.B) == spec["interleaved"], path
                # update blocks cross launches (or rounds of the one launch), masked launches sit between them
                assert info["ldlt_rounds"] >= 2 and info["ldlt_tasks"] >= 3, (path, info["ldlt_rounds"], info["ldlt_tasks"])
                if "single_launch" in spec:
                    rule = os.environ.get("SLPX_SINGLE_LAUNCH", "1" if self.B * info["ldlt_tasks"] <= 1024 else "0")[0] != "0"
                    assert rule == spec["single_launch"], path
        self.cache = {}

    def close(self):
        self.ls.close()
        if self.problem is not None:
            self.problem.p.close()


@pytest.fixture(scope="module")
def lasting_seams(slpx):
    made = {}

    def get(path):
        if path not in made:
            made[path] = Seam(slpx, path)
        return made[path]

    yield get
    for s in made.values():
        s.close()


@pytest.fixture()
def seam(request, slpx, lasting_seams):
    """The Seam of a path, made once per module under the path's switches.  (The pivoted dense one lives for one test:
    its model sits in the expression arena that other tests of this module clear.)"""
    path = request.param
    if PATHS[path].get("dense") == 2:
        s = Seam(slpx, path)
        yield s
        s.close()
    else:
        yield lasting_seams(path)


every_path = pytest.mark.parametrize("seam", PATH_IDS, indirect=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _batch(seam, seed=5):
    """(classes, right-hand sides) of the path's mixed batch."""
    cls = rm.batch_classes(seam.B)
    if seam.B >= 64:  # the last lane of the first wave of instances, the first and the last lane beyond it
        assert len({cls[63], cls[64], cls[seam.B - 1]}) == 3
    else:
        assert cls[2] == rm.GIVE_UP_CLASS
    return cls, rm.right_hand_sides(seam.B, seam.m.dim, seed)


def _compute(seam, cls, rhs, reset=True):
    """[reset,] set_matrix, set_rhs, compute(), the factorization's outputs, solve(), p."""
    ls = seam.ls
    if reset:
        ls.reset_regularization(1e-10)
    seam.set_matrix(seam.m.vals[cls])
    ls.set_rhs(rhs)
    info, reg, nfact = ls.compute()
    out = {"info": info.copy(), "reg": reg.copy(), "nfact": nfact}
    for k in FACTOR_OUTPUTS:
        out[k] = ls.get(k).copy()
    ls.solve()
    out["p"] = ls.get("p").copy()
    return out


def _mixed(seam):
    """The mixed batch from an empty memory, computed once per path (treat as read-only)."""
    if "mixed" not in seam.cache:
        cls, rhs = _batch(seam)
        seam.cache["mixed"] = (cls, rhs, _compute(seam, cls, rhs))
    return seam.cache["mixed"]


_KREG = {}


def _regularized_matrix(shape, c, d, g):
    """(K_reg, |K_reg|_inf, cond_2(K_reg), inertia) of a class at a regularization, computed once."""
    key = (shape, int(c), float(d), float(g))
    if key not in _KREG:
        m = rm.model(shape)
        Kreg = rm.regularized(m.K[int(c)], m.n, d, g)
        _KREG[key] = (Kreg, float(np.abs(Kreg).sum(axis=1).max()), float(np.linalg.cond(Kreg)), rm.inertia(m.K[int(c)], m.n, d, g)[0])
    return _KREG[key]


def _check_linear_algebra(seam, c, reg, rhs, x, D, where):
    """Assertion 2 for one instance with info = 0: inertia of K + reg by eigenvalues, the signs of D, the normwise
    backward error <= 1e-10, x against numpy.linalg.solve within max(1e-8, 2 kappa eta) — the rule and constants of
    test_config4_batch_items_match_oracle."""
    m = seam.m
    Kreg, k_inf, kappa, inertia = _regularized_matrix(seam.shape, c, reg[0], reg[1])
    assert inertia == (m.n, m.m_e, 0), (where, c, tuple(reg), inertia)
    assert (int((D > 0).sum()), int((D < 0).sum())) == (m.n, m.m_e), (where, c, tuple(reg))
    assert np.isfinite(x).all(), (where, c)
    eta = float(np.abs(Kreg @ x - rhs).max()) / max(1.0, float(np.abs(rhs).max()), k_inf * float(np.abs(x).max()))
    ref = np.linalg.solve(Kreg, rhs)
    err, tol = cases.max_rel(x, ref), max(1e-8, 2.0 * kappa * eta)
    assert eta <= 1e-10, (where, c, tuple(reg), eta)
    assert err <= tol, (where, c, tuple(reg), err, tol)
    return eta, err


def _check_decisions(seam, cls, out, prev, where):
    """Assertion 1: info, reg and the number of launches are expected()'s, exactly.  Returns the expectations."""
    exp = [rm.expected_of(seam.shape, c, 0.0 if prev is None else prev[b]) for b, c in enumerate(cls)]
    for b, e in enumerate(exp):
        assert out["info"][b] == e["info"], (where, b, cls[b], out["info"][b], e["info"])
        assert tuple(out["reg"][b]) == e["memory"], (where, b, cls[b], tuple(out["reg"][b]), e["memory"])
    assert out["nfact"] == max(len(e["attempts"]) for e in exp), (where, out["nfact"])
    return exp


def _check_all(seam, cls, out, rhs, where):
    worst = (0.0, 0.0)
    for b, c in enumerate(cls):
        if out["info"][b] == 0:
            eta, err = _check_linear_algebra(seam, c, out["reg"][b], rhs[b], out["p"][b], out["D"][b], (where, b))
            worst = (max(worst[0], eta), max(worst[1], err))
    return worst


@every_path
def test_decisions_and_solutions_of_a_mixed_batch(seam):
    """Assertions 1 and 2: every instance ends where expected() says — six different rungs and a give-up in one batch —
    after as many launches as the longest ladder (26: the unregularized attempt and delta = 1e-4 ... 1e20), and every
    accepted instance's factors and solution are those of ITS matrix at ITS regularization."""
    path = seam.path
    cls, rhs, out = _mixed(seam)
    exp = _check_decisions(seam, cls, out, None, path)
    assert out["nfact"] == 26 and {e["info"] for e in exp} == {0, 1}
    rungs = sorted({e["memory"] for e in exp if e["info"] == 0})
    assert len(rungs) >= (6 if seam.B >= 8 else 4)
    eta, err = _check_all(seam, cls, out, rhs, path)
    print(f"{path}: B = {seam.B}, rounds {seam.ls.info['ldlt_rounds']}, tasks {seam.ls.info['ldlt_tasks']}; rungs accepted "
          f"{[r[0] for r in rungs]} + give-up after {out['nfact']} launches; worst backward error {eta:.2e}, worst error {err:.2e}")


@every_path
def test_a_masked_lane_keeps_the_bits_of_an_unmasked_run(seam):
    """Assertion 3: against a batch of the same size whose instances are ALL of class c — every lane accepts in the
    same launch, nothing is ever masked — an instance of class c of the mixed batch (same place, same right-hand side)
    has L, D, z, its update blocks and p to the bit: same plan, same arithmetic per lane, only the masked launches in
    between differ."""
    path = seam.path
    cls, rhs, out = _mixed(seam)
    for c in sorted(set(cls)):
        alone = _compute(seam, np.full(seam.B, c), rhs)
        e = rm.expected_of(seam.shape, c)
        assert (alone["info"] == e["info"]).all() and alone["nfact"] == len(e["attempts"])
        for b in np.flatnonzero(cls == c):
            assert tuple(alone["reg"][b]) == tuple(out["reg"][b])
            for k in FACTOR_OUTPUTS + ("p",):
                assert _same_bits(out[k][b], alone[k][b]), (path, "class", c, "instance", b, k,
                                                            np.flatnonzero(_bits(out[k][b]) != _bits(alone[k][b]))[:8])


@every_path
def test_instances_do_not_notice_each_other(seam):
    """Assertion 4: the mixed batch under a permutation of its instances — every instance brings its info, reg, L, D, z,
    update blocks and p along to its new place, bit for bit."""
    path = seam.path
    cls, rhs, out = _mixed(seam)
    perm = np.random.default_rng(17).permutation(seam.B)
    assert (perm != np.arange(seam.B)).any() and (cls[perm] != cls).any()
    moved = _compute(seam, cls[perm], rhs[perm])
    assert moved["nfact"] == out["nfact"]
    for j, b in enumerate(perm):
        assert moved["info"][j] == out["info"][b] and tuple(moved["reg"][j]) == tuple(out["reg"][b]), (path, j, b)
        for k in FACTOR_OUTPUTS + ("p",):
            assert _same_bits(moved[k][j], out[k][b]), (path, "instance", b, "at", j, k)


@every_path
def test_the_memory_is_per_instance(seam):
    """Assertion 5: a second compute() without a reset starts every instance from ITS delta / 2; then the classes move on
    by one instance, so each instance meets another class with its own memory; then a new right-hand side on the kept
    factors."""
    path = seam.path
    cls, rhs = _batch(seam)
    first = _compute(seam, cls, rhs)
    _check_decisions(seam, cls, first, None, (path, "first"))
    second = _compute(seam, cls, rhs, reset=False)
    exp2 = _check_decisions(seam, cls, second, first["reg"][:, 0], (path, "second"))
    if seam.B >= 8:  # the two classes that shared delta = 1e-4 now differ
        assert {(5e-5, 1e-10), (5e-4, 1e-10)} <= {e["memory"] for e in exp2}
    _check_all(seam, cls, second, rhs, (path, "second"))
    moved = np.roll(cls, 1)
    assert (moved != cls).any()
    third = _compute(seam, moved, rhs, reset=False)
    exp3 = _check_decisions(seam, moved, third, second["reg"][:, 0], (path, "third"))
    _check_all(seam, moved, third, rhs, (path, "third"))
    # a new right-hand side on the factors in memory
    rhs2 = rm.right_hand_sides(seam.B, seam.m.dim, 6)
    seam.ls.set_rhs(rhs2)
    seam.ls.solve()
    third["p"] = seam.ls.get("p").copy()
    _check_all(seam, moved, third, rhs2, (path, "third, new right-hand side"))
    print(f"{path}: launches {first['nfact']} / {second['nfact']} / {third['nfact']}; rungs of the second compute "
          f"{sorted({e['memory'][0] for e in exp2})}, after the classes moved {sorted({e['memory'][0] for e in exp3})}")


@every_path
def test_the_mask_one_launch_at_a_time(seam):
    """Assertion 6: factor(d1, g) with every instance at its accepted rung (the give-up class at delta = 1), then
    factor(d2, g) with d2 = NaN for every other instance and 10 d1 for the rest: the NaN instances keep L, D, z and
    their update blocks to the bit, the others' counters show the inertia of 10 d1, and solve() then serves every
    instance with the factors of its own regularization."""
    path = seam.path
    m, B = seam.m, seam.B
    cls, rhs = _batch(seam)
    d1 = np.array([1.0 if c == rm.GIVE_UP_CLASS else rm.expected_of(seam.shape, c)["memory"][0] for c in cls])
    g = np.array([0.0 if c == 0 else 1e-10 for c in cls])
    masked = np.arange(B) % 2 == 0
    assert rm.GIVE_UP_CLASS in cls[masked] and len(set(cls[masked])) >= 3 and len(set(cls[~masked])) >= 2
    d2 = np.where(masked, np.nan, 10.0 * d1)
    seam.ls.reset_regularization(1e-10)
    seam.set_matrix(m.vals[cls])
    seam.ls.set_rhs(rhs)
    stats1 = seam.ls.factor(d1, g)
    before = {k: seam.ls.get(k).copy() for k in FACTOR_OUTPUTS}
    for b, c in enumerate(cls):
        assert tuple(int(v) for v in stats1[b, :4]) == rm.inertia(m.K[c], m.n, d1[b], g[b])[0] + (0,), (path, b, c, stats1[b])
    stats2 = seam.ls.factor(d2, g)
    after = {k: seam.ls.get(k).copy() for k in FACTOR_OUTPUTS}
    for b, c in enumerate(cls):
        if masked[b]:
            for k in FACTOR_OUTPUTS:
                assert _same_bits(after[k][b], before[k][b]), (path, "masked instance", b, "class", c, k)
        else:
            assert tuple(int(v) for v in stats2[b, :4]) == rm.inertia(m.K[c], m.n, d2[b], g[b])[0] + (0,), (path, b, c, stats2[b])
            if d2[b] != d1[b]:
                assert not _same_bits(after["D"][b], before["D"][b])
    seam.ls.solve()
    p = seam.ls.get("p")
    for b, c in enumerate(cls):
        if c != rm.GIVE_UP_CLASS:
            _check_linear_algebra(seam, c, (d1[b] if masked[b] else d2[b], g[b]), rhs[b], p[b], after["D"][b], (path, "after the masked launch", b))
