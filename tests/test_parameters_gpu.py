"""GPU tier of parameters as runtime inputs.  Every comparison is with the path that existed before: the same model
with the parameter values FOLDED IN — the variables hold the values when the model is compiled — and it is
np.array_equal throughout.  The equality is derived, not measured: the program, the code object and the inputs are the
same; only where a parameter's value comes from differs (its slot in the shared constant pool, rewritten in place, or in
the pool of its batch instance) and the kernels hold a batch to the same bits at any batch size
(tests/test_solve_batch_gpu.py::test_isolation_of_instances).

Models: tests/support/param_models.py (M2: Newton, Mq: SQP, chain(8): interior point with a generated body,
chain(4): interpreted tasks only).  Task classes exercised: the generated bodies, the interpreted 64-thread tasks riding
in their launch (chain(8)), tape_sweep_lds_kernel<64> on its own (chain(4); chain(8) under SLPX_TAPE_JIT=0 and
SLPX_TAPE_TEMPLATES=0).  The 256-thread and the global-memory classes take the same one-line change and are not
reached at these sizes; tests/test_tape_sweep_gpu.py::test_parameter_pool_per_instance reaches them."""
import numpy as np
import pytest

from tests.support import param_models as pmod

pytestmark = pytest.mark.gpu

SUCCESS, GLOBALLY_INFEASIBLE = 0, -3


@pytest.fixture
def m(fresh):
    mm = pmod.new_model()
    mm.be.reset()
    return mm


def _state(n, me, mi, batch, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (batch, n)), rng.uniform(0.5, 1.5, (batch, mi)), rng.uniform(-1, 1, (batch, me)),
            rng.uniform(0.5, 1.5, (batch, mi)))


# ---- 1. the sweep, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages,env", [(8, {}), (4, {}), (8, {"SLPX_TAPE_TEMPLATES": "0"}), (8, {"SLPX_TAPE_JIT": "0"})])
def test_sweep_with_a_pool_per_instance(m, slpx, monkeypatch, stages, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 3
    rows = pmod.chain_rows(stages, B)
    pm = pmod.chain(m, stages, rows[0])
    n, me, mi = pm.p.p.dims
    x, s, y, z = _state(n, me, mi, B, seed=stages)
    # today's path: a batch-1 system of a model compiled with the row folded in, at the same x and duals
    folded = []
    for b in range(B):
        pf = pmod.chain(m, stages, rows[b])
        sf = slpx.System(pf.p.p, batch=1)
        sf.set_state(x=x[b], s=s[b], y=y[b], z=z[b])
        sf.sweep(full=True)
        folded.append(sf.get("V")[0].copy())
        sf.sweep(full=False)
        assert np.array_equal(sf.get("V")[0], folded[b])  # (the values-only sweep rewrites f, c_e, c_i with the same bits)
        sf.close()
        pf.close()
    assert not np.array_equal(folded[0], folded[1]) and not np.array_equal(folded[1], folded[2])
    sys = slpx.System(pm.p.p, batch=B)
    sys.set_state(x=x, s=s, y=y, z=z)
    assert sys.parameter_pool_bytes() == 0
    sys.set_parameters(rows, per_instance=True)
    # two pools (full and values-only program), each B x (its constants: the parameters and some literals)
    assert sys.parameter_pool_bytes() % (8 * B) == 0 and sys.parameter_pool_bytes() >= 2 * 8 * B * rows.shape[1]
    sys.sweep(full=True)
    V = sys.get("V")
    for b in range(B):
        assert np.array_equal(V[b], folded[b]), (b, np.flatnonzero(V[b] != folded[b])[:8])
    # the values-only program reads its own per-instance pool
    sys.set_state(x=x[::-1].copy(), s=s, y=y, z=z)
    sys.sweep(full=True)
    sys.set_state(x=x, s=s, y=y, z=z)
    sys.sweep(full=False)
    info = sys.info
    head = 1 + info["m_e"] + info["m_i"]
    V = sys.get("V")
    for b in range(B):
        assert np.array_equal(V[b][:head], folded[b][:head]), b
    # a shared install: every instance is the model with that row
    for row_b in (1, 2):
        sys.set_parameters(rows[row_b], per_instance=False)
        sys.set_state(x=np.repeat(x[row_b][None], B, 0), s=np.repeat(s[row_b][None], B, 0),
                      y=np.repeat(y[row_b][None], B, 0), z=np.repeat(z[row_b][None], B, 0))
        sys.sweep(full=True)
        V = sys.get("V")
        for b in range(B):
            assert np.array_equal(V[b], folded[row_b]), (row_b, b)
    sys.close()
    pm.close()


# ---- 2. re-solve without a recompile -------------------------------------------------------------------------------
def _solve_record(p):
    status, rep = p.solve()
    s, y, z = p.duals()
    return {"status": status, "iterations": rep["iterations"], "x": p.get_x(), "s": s, "y": y, "z": z}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, a[k], b[k])


RESOLVE_CASES = {
    "m2": (lambda m, row: pmod.m2(m, row), [(2.0,), (-1.5,), (0.25,)]),
    "mq": (lambda m, row: pmod.mq(m, row), [(2.0, 1.0), (-1.0, 3.0), (0.5, -2.0)]),
    "chain8": (lambda m, row: pmod.chain(m, 8, row), list(pmod.chain_rows(8, 3))),
}


@pytest.mark.parametrize("case", list(RESOLVE_CASES))
def test_resolve_without_a_recompile(m, slpx, case):
    build, rows = RESOLVE_CASES[case]
    pm = build(m, rows[0])
    p = pm.p.p
    x_start = p.get_x()
    first = _solve_record(p)
    assert first["status"] == SUCCESS and p.compile_count() == 1
    handle = p.system()  # taken BEFORE the parameters change
    p.set_parameters(rows[1])
    assert p.compile_count() == 1
    assert [pm.p.be.value(i) for i in pm.param_ids] == [float(v) for v in rows[1]]  # the variables have the values too
    p.set_x(x_start)
    second = _solve_record(p)
    assert p.compile_count() == 1, "set_parameters + solve compiled again"
    # a fresh problem built with the new values, from the same start
    fresh_pm = build(m, rows[1])
    fresh_pm.p.p.set_x(x_start)
    want = _solve_record(fresh_pm.p.p)
    _same(second, want, case + ": set_parameters vs a fresh model")
    assert not np.array_equal(second["x"], first["x"])
    # the handle taken before still drives the system the problem solves on, with the new values
    n, me, mi = p.dims
    x, s, y, z = _state(n, me, mi, 1, seed=3)
    fresh_sys = fresh_pm.p.p.system()
    for sy in (handle, fresh_sys):
        sy.set_scaling(np.ones(1 + me + mi))
        sy.set_state(x=x, s=s, y=y, z=z)
        sy.sweep(full=True)
    assert np.array_equal(handle.get("V"), fresh_sys.get("V"))
    assert p.compile_count() == 1
    fresh_pm.close()
    # set_value on a parameter keeps its old meaning: the next solve notices and compiles a new system
    pm.p.be.set_value(pm.param_ids[0], float(rows[2][0]))
    p.set_x(x_start)
    third = _solve_record(p)
    assert p.compile_count() == 2
    row3 = np.array(rows[1], dtype=np.float64)
    row3[0] = rows[2][0]
    fresh_pm = build(m, row3)
    fresh_pm.p.p.set_x(x_start)
    _same(third, _solve_record(fresh_pm.p.p), case + ": set_value vs a fresh model")
    # ... and set_parameters keeps working on the new system
    p.set_parameters(rows[0])
    p.set_x(x_start)
    _same(_solve_record(p), first, case + ": back to the first values")
    assert p.compile_count() == 2
    fresh_pm.close()
    pm.close()


# ---- 3. a batch with a parameter row per instance = B separate models -----------------------------------------------
BATCH_CASES = {
    # (quadratic programs: one step from anywhere — and none from the solution, where the last instance of each starts)
    "m2": (lambda m, row: pmod.m2(m, row), np.array([[2.0], [-1.5], [40.0], [0.0]]),
           np.array([[0.0, 0.0], [1.0, -1.0], [0.5, 0.5], [0.0, 1.0]])),
    "mq": (lambda m, row: pmod.mq(m, row), np.array([[2.0, 1.0], [-1.0, 3.0], [0.5, -2.0], [2.0, 3.0]]),
           np.array([[0.0, 0.0], [1.0, -1.0], [0.5, 0.5], [2.0, 1.0]])),
    "chain8": (lambda m, row: pmod.chain(m, 8, row), pmod.chain_rows(8, 4), None),
}


@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_batch_with_parameter_rows_equals_separate_models(m, case):
    build, rows, x0 = BATCH_CASES[case]
    B = len(rows)
    pm = build(m, rows[0])
    p = pm.p.p
    n = p.dims[0]
    if x0 is None:
        x0 = np.random.default_rng(11).uniform(-0.5, 0.5, (B, n))
    r = p.solve_batch(x0, parameters=rows)
    want = [pmod.folded_instance(lambda row: build(m, row), rows[b], x0[b], B) for b in range(B)]
    for b in range(B):
        pmod.assert_instance_equal(r, b, want[b], case)
    print(case, "iterations", r["iterations"], "status", r["status"])
    assert all(w["status"] == SUCCESS for w in want)
    assert len({int(w["iterations"]) for w in want}) >= 2, "the rows should not all take the same number of iterations"
    # no rows: exactly solve_batch
    plain, none = p.solve_batch(x0), p.solve_batch(x0, parameters=None)
    for k in pmod.BATCH_KEYS:
        assert np.array_equal(plain[k], none[k]), k
    pmod.assert_instance_equal(plain, 0, pmod.folded_instance(lambda row: build(m, row), rows[0], x0[0], B), case + " shared")
    # the shared pool is in force again, on the batch-1 system too: solve() gives what it gave
    assert [pm.p.be.value(i) for i in pm.param_ids] == [float(v) for v in rows[0]]
    p.set_x(np.zeros(n))
    again = _solve_record(p)
    _same(again, _solve_record_from(build, m, rows[0], np.zeros(n)), case + ": solve() after the batch")
    assert p.compile_count() == 1
    pm.close()


def _solve_record_from(build, m, row, x_start):
    pm = build(m, row)
    pm.p.p.set_x(x_start)
    rec = _solve_record(pm.p.p)
    pm.close()
    return rec


# ---- 4. restoration with parameters --------------------------------------------------------------------------------
RESTORING_ROWS = np.array([[1.0], [1.5], [0.75], [1.0]])
RESTORING_STARTS = np.array([[-4.0, 3.0, 1.0], [-3.0, 3.0, 1.0], [-2.0, 3.0, 1.0], [2.0, 3.0, 1.0]])


@pytest.mark.parametrize("mode", ["handoff", "lockstep"])
def test_restoration_with_parameter_rows(m, mode):
    """What catches a batch-1 system that works for an instance with another instance's parameters: the hand-off, the
    multiplier estimate and the KKT-error fallback all run there."""
    B = len(RESTORING_ROWS)
    build = lambda row: pmod.restoring(m, row)
    want = [pmod.folded_instance(build, RESTORING_ROWS[b], RESTORING_STARTS[b], B, restoration=mode) for b in range(B)]
    print(mode, "folded: restorations", [int(w["restorations"]) for w in want], "status", [int(w["status"]) for w in want],
          "iterations", [int(w["iterations"]) for w in want])
    assert sum(int(w["restorations"]) for w in want) > 0, "no row restores: the test would not reach the batch-1 system"
    restoring_rows = {float(RESTORING_ROWS[b][0]) for b in range(B) if want[b]["restorations"] > 0}
    assert restoring_rows - {float(RESTORING_ROWS[0][0])}, "only the problem's own row restores: a wrong row would not show"
    pm = build(RESTORING_ROWS[0])
    r = pm.p.p.solve_batch(RESTORING_STARTS, parameters=RESTORING_ROWS, restoration=mode)
    for b in range(B):
        pmod.assert_instance_equal(r, b, want[b], mode)
        assert r["restorations"][b] == want[b]["restorations"]
    # the batch-1 system has the problem's own values again
    pm.p.p.set_x(RESTORING_STARTS[0])
    _same(_solve_record(pm.p.p), _solve_record_from(lambda mm, row: pmod.restoring(mm, row), m, RESTORING_ROWS[0], RESTORING_STARTS[0]),
          mode + ": solve() after the batch")
    pm.close()


# ---- 5. a bound conflict of one instance ---------------------------------------------------------------------------
def test_bound_conflict_per_instance(m):
    rows = np.array([[0.0, 1.0], [2.0, 1.0], [-1.0, 5.0]])  # lo, hi: row 1 has lo > hi
    x0 = np.array([[0.5], [1.5], [0.0]])
    pm = pmod.boxed(m, rows[0])
    r = pm.p.p.solve_batch(x0, parameters=rows)
    assert list(r["status"]) == [SUCCESS, GLOBALLY_INFEASIBLE, SUCCESS]
    assert np.array_equal(r["x"][1], x0[1]) and r["iterations"][1] == 0
    for b in (0, 2):
        pmod.assert_instance_equal(r, b, pmod.folded_instance(lambda row: pmod.boxed(m, row), rows[b], x0[b], 3), "boxed")
    assert abs(r["x"][0][0] - 1.0) <= 1e-6 and abs(r["x"][2][0] - 3.0) <= 1e-6
    # the folded model of the conflicting row says the same, for all its instances
    bad = pmod.folded_instance(lambda row: pmod.boxed(m, row), rows[1], x0[1], 3)
    assert bad["status"] == GLOBALLY_INFEASIBLE and bad["cost"] == r["cost"][1]
    # without rows the verdict is the whole batch's, as before
    assert list(pm.p.p.solve_batch(x0)["status"]) == [SUCCESS] * 3
    pm.close()


def test_rows_for_a_model_without_parameters_are_refused(m, slpx):
    from tests.support import model

    p = model.NlpProblem(m)
    x = p.decision_variable(1.0)
    p.minimize(m.pow(x - 2, 2))
    L = slpx.lib()
    x0, rows = np.zeros((2, 1)), np.zeros((2, 1))
    rc = L.slpx_problem_solve_batch_parameters(p.p._h, 2, x0.ctypes.data, rows.ctypes.data, None, 0, *([None] * 8), None)
    assert rc == -100 and b"the model has none" in L.slpx_last_error()
    sy = slpx.System(p.p, batch=2)
    with pytest.raises(slpx.SlpxError):
        sy.set_parameters(rows, per_instance=True)
    assert L.slpx_system_set_parameters(sy._h, rows.ctypes.data, 2) == -100
    sy.close()
    p.p.close()


# ---- 6. the Python surface ------------------------------------------------------------------------------------------
def test_python_surface(fresh):
    from sleipnir_amd import autodiff, optimization

    p = optimization.Problem()
    x, y = p.decision_variable(), p.decision_variable()
    a = autodiff.Variable()
    a.set_value(2.0)
    p.minimize((x - a) ** 2 + (y - 1) ** 2)
    assert [v.node for v in p.parameters()] == [a.node]
    assert p.solve() == optimization.ExitStatus.SUCCESS
    assert abs(x.value() - 2.0) <= 1e-8 and abs(y.value() - 1.0) <= 1e-8
    p.set_parameters([-3.0])
    assert a.value() == -3.0
    assert p.solve() == optimization.ExitStatus.SUCCESS
    assert abs(x.value() + 3.0) <= 1e-8
    assert p._p.compile_count() == 1
    rows = np.array([[1.0], [5.0], [-2.0]])
    r = p.solve_batch(np.zeros((3, 2)), parameters=rows)
    assert all(s == optimization.ExitStatus.SUCCESS for s in r.status)
    assert np.max(np.abs(r.x[:, 0] - rows[:, 0])) <= 1e-8 and np.max(np.abs(r.x[:, 1] - 1.0)) <= 1e-8
    assert a.value() == -3.0 and p._p.compile_count() == 1
    p.close()
