"""The two kernels of a batched warm start (warm_start_batch_kernels.h) through their launch wrappers
(BatchDevice::warm_start, BatchDevice::unscaled_iterate), instance by instance: a probe (tests/support/warmcheck.cpp)
drives them on the batch system of a model (`sa.System(problem, B)`), and every output is compared with the numpy
restatement of warm_start.h in tests/support/warmcheck_host.py.  The c_i the kernel reads from the system's V, the scales
and the given blocks are set by the test, so each instance is a function of its number alone.

Tolerances:
  * s, y, z of the first iterate, the repair count, the non-finite flag, and the un-scaled iterate: bit for bit (each
    entry is single IEEE operations: a multiplication or a division per conversion, mu / s, the clamp's comparisons);
  * the first barrier parameter where it is the mean of s_j z_j: 1e-12 of the sum of the terms' magnitudes over the
    count — the figure of test_solve_batch_kernels_gpu.py for every batched sum (the device sums strided partials
    through block_reduce and may contract s z into the sum, numpy sums in np.longdouble).  Given or cold: exact.  The
    vectors that depend on it (max(c_i, mu), mu / s, the clamp) are compared at the DEVICE's value of it;
  * everything of one instance is bit for bit the same at slot 0 of B = 1, in B = 3 and in B = 17, under another mask,
    and from one run to the next;
  * an instance that is masked out, or whose input is not finite, keeps every bit of its iterate.
"""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import sleipnir_amd as sa
from tests.support import fr_models, model
from tests.support import param_models as pmod
from tests.support import warmcheck as wc
from tests.support import warmcheck_host as wh

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
TOLERANCE = 1e-8  # the solve's, for mu_min = d_f tolerance / 10


def _one(m):  # n = 1, m_e = 0, m_i = 1
    p = model.NlpProblem(m)
    x = p.decision_variable(0.5)
    p.minimize(m.pow(x - 3, 2))
    p.le(x, 1)
    return p.p


SHAPES = {
    "one": _one,                                             # m_i = 1, m_e = 0
    "boxed": lambda m: pmod.boxed(m, (0.0, 1.0)).p.p,        # m_i = 2, m_e = 0
    "restoring": lambda m: pmod.restoring(m, (1.0,)).p.p,    # m_i = 2, m_e = 2
    "mq": lambda m: pmod.mq(m, (2.0, 1.0)).p.p,              # m_i = 0, m_e = 1: BatchEqDevice
    "chain128": lambda m: fr_models.chain(m, 128).p,         # m_i = 278 (more rows than the workgroup has lanes), m_e = 62
}

_rigs = {}


class Rig:
    def __init__(self, name):
        m = model.Model(model.ProductBackend("gpu"))
        self.problem = SHAPES[name](m)
        self.systems = {}

    def probe(self, B):
        if B not in self.systems:
            system = sa.System(self.problem, B)
            self.systems[B] = (system, wc.WarmProbe(system))
        return self.systems[B][1]


@pytest.fixture(scope="module")
def probes():
    sa.lib().slpx_graph_reset()
    wc.lib()

    def rig(name):
        if name not in _rigs:
            _rigs[name] = Rig(name)
        return _rigs[name]

    yield rig
    for r in _rigs.values():
        for system, probe in r.systems.values():
            probe.close()
            system.close()
        r.problem.close()
    _rigs.clear()
    sa.lib().slpx_graph_reset()


def instance(k, n, m_e, m_i, nan_in=None):
    """Instance k: everything of it depends on k alone.  Rows with s <= 0, z <= 0, z outside the clamp; every third
    instance has scales of 1, every third a given mu."""
    rng = np.random.default_rng(4242 + 7919 * k)
    ns = 1 + m_e + m_i
    scales = np.ones(ns) if k % 3 == 0 else rng.uniform(0.2, 1.0, ns)
    x = rng.standard_normal(n)
    ci = 2.0 * rng.standard_normal(m_i)
    s = 10.0 ** rng.uniform(-9, 1, m_i)
    z = 10.0 ** rng.uniform(-9, 1, m_i)
    y = rng.standard_normal(m_e) * 10.0 ** rng.uniform(-3, 3, m_e)
    kind = rng.integers(0, 6, m_i)
    s[kind == 0] = 0.0
    s[kind == 1] *= -1.0
    z[kind == 2] = 0.0
    z[kind == 3] *= -1.0
    far = rng.integers(0, 8, m_i)
    z[far == 0] *= 1e-14  # below the clamp
    z[far == 1] *= 1e14   # above it
    mu = 10.0 ** rng.uniform(-7, -1) if k % 3 == 1 else (-1.0 if k % 3 == 2 else 0.0)
    d = dict(scales=scales, x=x, ci=ci, s=s, y=y, z=z, mu=mu, mu_min=scales[0] * TOLERANCE / 10.0)
    if nan_in is not None:
        d = {key: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for key, v in d.items()}
        if nan_in == "mu":
            d["mu"] = float("inf")
        else:
            d[nan_in][-1] = float("nan")
    return d


def run_batch(probe, insts, present, run):
    """One launch of batch_warm_start_kernel on the instances `insts` (slot order) with the blocks in `present` given.
    -> (out [B][3], s, y, z of the iterate afterwards)"""
    B, n, m_e, m_i = probe.B, probe.n, probe.m_e, probe.m_i
    assert len(insts) == B
    stack = lambda key, k: np.array([i[key] for i in insts]).reshape(B, k)
    probe.set_scales(stack("scales", probe.ns))
    probe.set_iterate(stack("x", n), np.full((B, m_i), SENTINEL), np.full((B, m_e), SENTINEL), np.full((B, m_i), SENTINEL))
    probe.set_ci(stack("ci", m_i))
    blocks = [stack(key, k) if key in present else None for key, k in (("s", m_i), ("y", m_e), ("z", m_i), ("mu", 1))]
    out = probe.warm_start(*blocks, run, stack("mu_min", 1))
    _, s, y, z = probe.get_iterate()
    return out, s, y, z


def check_instance(inst, present, m_e, out, s, y, z, what):
    g = lambda key: inst[key] if key in present else None
    mu_given = inst["mu"] if "mu" in present else 0.0
    ref = wh.instance(inst["scales"], m_e, inst["ci"], inst["x"], g("s"), g("y"), g("z"), mu_given, inst["mu_min"])
    if ref["bad"]:
        assert list(out) == [0.0, 0.0, 1.0], (what, out)
        for v in (s, y, z):
            assert np.all(v == SENTINEL), what
        return
    assert out[2] == 0.0, (what, out)
    if mu_given > 0.0 or ref["count"] == 0:
        assert out[0] == ref["mu"], (what, out[0], ref["mu"])
    else:
        mag = ref["sum"] / ref["count"]
        assert abs(out[0] - ref["mu"]) <= 1e-12 * max(mag, abs(ref["mu"])), (what, out[0], ref["mu"])
    ref = wh.instance(inst["scales"], m_e, inst["ci"], inst["x"], g("s"), g("y"), g("z"), mu_given, inst["mu_min"],
                      mu=out[0])
    assert out[1] == ref["repaired"], (what, out[1], ref["repaired"])
    for name, dev, want in (("s", s, ref["s"]), ("y", y, ref["y"]), ("z", z, ref["z"])):
        assert np.array_equal(dev.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (what, name, dev, want)


BLOCKS = ("s", "y", "z", "mu")
ALL_COMBOS = [frozenset(c) for r in range(5) for c in itertools.combinations(BLOCKS, r)]
# every combination of absent blocks on the model with both kinds of rows and on the one with more rows than lanes; the
# others: all given, the duals only, the slacks only
SOME_COMBOS = [frozenset(BLOCKS), frozenset(("y", "z")), frozenset(("s", "mu"))]


@pytest.mark.parametrize("name,combos", [("restoring", ALL_COMBOS), ("chain128", ALL_COMBOS), ("one", SOME_COMBOS),
                                         ("boxed", SOME_COMBOS), ("mq", SOME_COMBOS)])
def test_warm_start_kernel(probes, name, combos):
    r = probes(name)
    p17, p3, p1 = r.probe(17), r.probe(3), r.probe(1)
    n, m_e, m_i = p17.n, p17.m_e, p17.m_i
    saw_repair = saw_clean = False
    for present in combos:
        # where the non-finite entry sits: in a given block of this model, else in x
        nan_in = next((k for k in ("z", "y", "s", "mu") if k in present and (k == "mu" or {"s": m_i, "y": m_e, "z": m_i}[k])), "x")
        if m_i == 0 and nan_in == "mu":
            nan_in = "x"  # (without inequality rows mu is not read)
        insts = [instance(k, n, m_e, m_i, nan_in if k == 5 else None) for k in range(17)]
        run17 = np.ones(17, dtype=np.uint8)
        run17[9] = 0
        what = (name, sorted(present))
        out, s, y, z = run_batch(p17, insts, present, run17)
        for b in range(17):
            if b == 9:  # masked out: every bit stays (the out row is the zero the launch starts from)
                assert list(out[b]) == [0.0, 0.0, 0.0] and all(np.all(v[b] == SENTINEL) for v in (s, y, z)), what
                continue
            check_instance(insts[b], present, m_e, out[b], s[b], y[b], z[b], what + (b,))
            saw_repair = saw_repair or out[b][1] > 0
            saw_clean = saw_clean or (out[b][2] == 0 and out[b][1] == 0)
        assert out[5][2] == 1.0, what
        # the same bits in a second run, ...
        again = run_batch(p17, insts, present, run17)
        for a, b in zip((out, s, y, z), again):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what
        # ... in other slots of a smaller batch under another mask (the instance masked above runs here), and alone
        slots = [16, 9, 7]
        o3, s3, y3, z3 = run_batch(p3, [insts[k] for k in slots], present, np.array([1, 1, 1], dtype=np.uint8))
        check_instance(insts[9], present, m_e, o3[1], s3[1], y3[1], z3[1], what + ("B=3", 9))
        for j, k in ((0, 16), (2, 7)):
            for a, b in ((o3, out), (s3, s), (y3, y), (z3, z)):
                assert np.array_equal(a[j].view(np.uint64), b[k].view(np.uint64)), what + ("B=3", k)
        o1, s1, y1, z1 = run_batch(p1, [insts[7]], present, np.array([1], dtype=np.uint8))
        for a, b in ((o1, out), (s1, s), (y1, y), (z1, z)):
            assert np.array_equal(a[0].view(np.uint64), b[7].view(np.uint64)), what + ("B=1",)
    if m_i:
        assert saw_repair  # (the instances do reach the repairs)


def test_a_converged_iterate_passes_untouched(probes):
    """s z = mu on every row, active (s ~ 1e-9) and inactive (z ~ 1e-9) alike, scales of 1: no repair, every bit kept."""
    p = probes("chain128").probe(3)
    B, n, m_e, m_i = p.B, p.n, p.m_e, p.m_i
    rng = np.random.default_rng(5)
    mu = 1e-9
    s = np.where(rng.integers(0, 2, (B, m_i)) == 0, 1e-9, 1.0) * rng.uniform(0.5, 2.0, (B, m_i))
    z = mu / s
    y = rng.standard_normal((B, m_e))
    p.set_scales(np.ones((B, p.ns)))
    p.set_iterate(rng.standard_normal((B, n)), np.full((B, m_i), SENTINEL), np.full((B, m_e), SENTINEL), np.full((B, m_i), SENTINEL))
    p.set_ci(s)
    out = p.warm_start(s, y, z, np.full(B, mu), np.ones(B, dtype=np.uint8), np.full(B, 1e-9))
    _, ds, dy, dz = p.get_iterate()
    assert np.array_equal(out, np.array([[mu, 0.0, 0.0]] * B))
    for dev, want in ((ds, s), (dy, y), (dz, z)):
        assert np.array_equal(dev.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", ["restoring", "chain128", "mq", "one"])
def test_unscale_kernel(probes, name):
    """s / d_ci, y (d_ce / d_f), z (d_ci / d_f): exact against numpy; a masked instance's outputs stay 0."""
    r = probes(name)
    for B in (1, 3, 17):
        p = r.probe(B)
        n, m_e, m_i = p.n, p.m_e, p.m_i
        insts = [instance(k, n, m_e, m_i) for k in range(B)]
        stack = lambda key, k: np.array([i[key] for i in insts]).reshape(B, k)
        p.set_scales(stack("scales", p.ns))
        p.set_iterate(stack("x", n), stack("s", m_i), stack("y", m_e), stack("z", m_i))
        run = np.ones(B, dtype=np.uint8)
        if B > 1:
            run[1] = 0
        s_u, y_u, z_u = p.unscaled_iterate(run)
        for b, inst in enumerate(insts):
            sc = inst["scales"]
            d_f, d_ce, d_ci = sc[0], sc[1:1 + m_e], sc[1 + m_e:]
            want = (wh.unscale_s(inst["s"], d_ci), wh.unscale_dual(inst["y"], d_ce, d_f), wh.unscale_dual(inst["z"], d_ci, d_f))
            if not run[b]:
                want = tuple(np.zeros_like(w) for w in want)
            for dev, w in zip((s_u[b], y_u[b], z_u[b]), want):
                assert np.array_equal(dev.view(np.uint64), np.ascontiguousarray(w, dtype=np.float64).view(np.uint64)), (name, B, b)
            if run[b] and b % 3 == 0:  # scales of 1: the iterate's own bits
                assert np.array_equal(s_u[b], inst["s"]) and np.array_equal(z_u[b], inst["z"])
