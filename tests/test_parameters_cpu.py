"""CPU tier of parameters as runtime inputs: what can be said about a model's parameters without a device
(slpx_problem_parameters, slpx_problem_parameter_slots_in_order: the host-only structure path of
slpx_problem_prebuild_kernels), the error conventions of the new entry points, and that the generated kernel of a
model with parameters still cross-compiles for gfx950.

Models: tests/support/param_models.py."""
import ctypes

import numpy as np
import pytest

from tests.support import param_models as pmod


@pytest.fixture
def m(fresh):
    mm = pmod.new_model()
    mm.be.reset()
    return mm


@pytest.mark.parametrize("stages", [8, 4])
def test_parameters_of_the_chain(m, stages):
    """The count, the ids in ascending node order, and no decision variable among them — although decision variables
    and parameters are both free variables of the graph, created here in turn."""
    rows = pmod.chain_rows(stages, 1)
    pm = pmod.chain(m, stages, rows[0])
    ids = pm.p.p.parameters()
    assert len(ids) == pmod.chain_parameter_count(stages)
    assert ids == sorted(ids)
    assert ids == pm.param_ids  # (created in ascending order by the builder)
    assert not set(ids) & {v.node for v in pm.x}
    # capacity is respected, the count is the answer either way
    L = pm.p.be.L
    few = np.full(4, -1, dtype=np.int32)
    assert L.slpx_problem_parameters(pm.p.p._h, few.ctypes.data, 2) == len(ids)
    assert list(few) == ids[:2] + [-1, -1]
    assert pm.p.p.compile_count() == 0  # nothing was compiled for the device
    pm.close()


@pytest.mark.parametrize("stages", [8, 4])
def test_slot_of_parameter_j_is_j_in_both_programs(m, stages, monkeypatch):
    """tape_compiler.cpp hands out the parameters' constant slots first and in node order, in the full program and in
    the values-only program alike — with the families of the template compiler and with the flat compiler."""
    pm = pmod.chain(m, stages, pmod.chain_rows(stages, 1)[0])
    assert pm.p.p.parameter_slots_in_order()
    monkeypatch.setenv("SLPX_TAPE_TEMPLATES", "0")
    assert pm.p.p.parameter_slots_in_order()
    assert pm.p.p.parameters() == pm.param_ids
    pm.close()


def test_a_parameter_nothing_reaches_is_not_listed(m):
    pm = pmod.mq(m, (2.0, 1.0))
    unused = m.variable(5.0)
    assert pm.p.p.parameters() == pm.param_ids and unused.node not in pm.p.p.parameters()
    pm.close()


def test_a_model_without_parameters_has_none(m):
    from tests.support import model

    p = model.NlpProblem(m)
    x = p.decision_variable(1.0)
    p.minimize(m.pow(x - 2, 2))
    assert p.p.parameters() == []
    assert p.p.parameter_slots_in_order()
    p.p.close()


def test_errors_follow_the_neighbours(m, slpx):
    """-100 + slpx_last_error for a null problem / null arrays; the count query answers -100 too; a null problem has
    compile count -1."""
    L = slpx.lib()
    pm = pmod.m2(m, (2.0,))
    assert L.slpx_problem_parameters(None, None, 0) == -100 and b"null problem" in L.slpx_last_error()
    assert L.slpx_problem_set_parameters(None, None) == -100 and b"null problem" in L.slpx_last_error()
    assert L.slpx_problem_set_parameters(pm.p.p._h, None) == -100 and b"values is null" in L.slpx_last_error()
    assert L.slpx_system_set_parameters(None, None, 0) == -100 and b"null system" in L.slpx_last_error()
    assert L.slpx_problem_compile_count(None) == -1
    x0 = np.zeros((1, 2))
    rc = L.slpx_problem_solve_batch_parameters(None, 1, x0.ctypes.data, None, None, 0, *([None] * 8), None)
    assert rc == -100 and b"null problem" in L.slpx_last_error()
    with pytest.raises(ValueError):
        pm.p.p.solve_batch(x0, parameters=np.zeros((2, 1)))  # one row per instance
    with pytest.raises(ValueError):
        pm.p.p.solve_batch(x0, parameters=np.zeros((1, 3)))  # one column per parameter
    with pytest.raises(ValueError):
        pm.p.p.set_parameters([1.0, 2.0])
    pm.close()


def test_generated_kernel_of_a_model_with_parameters_compiles(m, tmp_path):
    """The 8-stage chain's dynamics rows are a family with a generated body whose constant loads go through the
    per-instance pool address (tape_jit.cpp); the 4-stage chain has no family.  hipRTC cross-compiles without a GPU."""
    pm = pmod.chain(m, 8, pmod.chain_rows(8, 1)[0])
    assert pm.p.p.prebuild_kernels(tmp_path / "c8") >= 1
    pm.close()
    pm = pmod.chain(m, 4, pmod.chain_rows(4, 1)[0])
    assert pm.p.p.prebuild_kernels(tmp_path / "c4") == 0
    pm.close()


def test_python_surface_without_a_device(fresh):
    """optimization.Problem.parameters() names the Variables; an unknown keyword of solve_batch stays a KeyError."""
    from sleipnir_amd import autodiff, optimization

    p = optimization.Problem()
    x, y = p.decision_variable(), p.decision_variable()
    a = autodiff.Variable()  # (a free variable; Variable(2.0) would be a constant)
    a.set_value(2.0)
    p.minimize((x - a) ** 2 + (y - 1) ** 2)
    assert [v.node for v in p.parameters()] == [a.node]
    with pytest.raises(KeyError):
        p.solve_batch(np.zeros((1, 2)), parameter=np.zeros((1, 1)))
    p.close()
