"""The reference's Python interface `sleipnir.optimization`
(python/cpp/optimization/bind_problem.cpp:30-160, bind_ocp.cpp:25-130,
solver/bind_exit_status.cpp, solver/bind_iteration_info.cpp,
python/src/sleipnir/optimization/__init__.py:6-31) over the C-ABI of libslpx: Problem, OCP,
ExitStatus, bounds, the constraint types and multistart with the reference's names, argument
meaning and error behaviour.  solve() runs Problem::solve of the library (interior point, SQP
or Newton by the kinds of constraints present, problem.hpp:335,403,512) on the MI355X; there is
no CPU fallback — without a HIP device it raises.
"""
from __future__ import annotations

import concurrent.futures
import dataclasses
import enum
import math

import numpy as np

import sleipnir_amd as _sa
from sleipnir_amd.autodiff import (EqualityConstraints, ExpressionType, InequalityConstraints, Variable,
                                   VariableMatrix, _is_scalar)

__all__ = ["ExitStatus", "Problem", "OCP", "DynamicsType", "TimestepMethod", "TranscriptionMethod",
           "EqualityConstraints", "InequalityConstraints", "IterationInfo", "bounds", "multistart",
           "Iterate", "BatchIterate", "BatchResult", "Sensitivity", "BatchSensitivity", "Cotangent"]


class ExitStatus(enum.IntEnum):
    """solver/exit_status.hpp:13-43"""
    SUCCESS = 0
    CALLBACK_REQUESTED_STOP = 1
    TOO_FEW_DOFS = -1
    LOCALLY_INFEASIBLE = -2
    GLOBALLY_INFEASIBLE = -3
    FACTORIZATION_FAILED = -4
    LINE_SEARCH_FAILED = -5
    FEASIBILITY_RESTORATION_FAILED = -6
    NONFINITE_INITIAL_GUESS = -7
    DIVERGING_ITERATES = -8
    MAX_ITERATIONS_EXCEEDED = -9
    TIMEOUT = -10


def bounds(l, x, u) -> InequalityConstraints:
    """variable.hpp:1008-1013: l <= x <= u"""
    return InequalityConstraints([l <= x, x <= u])


class IterationInfo:
    """solver/iteration_info.hpp:13-41: iteration, x, s, y, z as arrays; g, H, A_e, A_i as scipy
    matrices over the static patterns (built when asked for)."""

    def __init__(self, raw, problem):
        self.iteration = raw["iteration"]
        self.x, self.s, self.y, self.z = raw["x"], raw["s"], raw["y"], raw["z"]
        self.in_restoration = raw["in_restoration"]
        self._raw, self._problem = raw, problem
        # the value vector belongs to the solver: copy what the properties below need now
        self._V = None
        if not self.in_restoration:
            end = problem._value_count()
            if end:
                self._V = np.ctypeslib.as_array(raw["V"], shape=(end,)).copy()

    def _matrix(self, which, off_index, shape, lower=False):
        import scipy.sparse

        if self._V is None:
            raise RuntimeError("matrices are not available inside feasibility restoration")
        cp, ri = self._problem._patterns()[which]
        off = self._raw["off"][off_index]
        nnz = int(cp[-1])
        m = scipy.sparse.csc_matrix((self._V[off:off + nnz], np.asarray(ri[:nnz]), np.asarray(cp)), shape=shape)
        m.sum_duplicates()
        return m

    @property
    def g(self):
        n = len(self.x)
        return self._matrix(0, 3, (1, n)).T.tocsc()

    @property
    def A_e(self):
        return self._matrix(1, 4, (len(self.y), len(self.x)))

    @property
    def A_i(self):
        return self._matrix(2, 5, (len(self.z), len(self.x)))

    @property
    def H(self):
        """Hessian of the Lagrangian, lower triangle (iteration_info.hpp:34): H_f + H_c"""
        n = len(self.x)
        return (self._matrix(3, 6, (n, n)) + self._matrix(4, 7, (n, n))).tocsc()


@dataclasses.dataclass
class Iterate:
    """A primal-dual iterate in the user's units, whatever scaling the solve ran with: x, the slacks s of the
    inequality constraints, the multipliers y, z of f - y^T c_e - z^T c_i as the model was written, and the barrier
    parameter mu.  What Problem.iterate() returns and Problem.solve(warm_start=...) takes; any of s, y, z may be None
    (absent) and mu None or <= 0 (chosen from s and z)."""
    x: object = None
    s: object = None
    y: object = None
    z: object = None
    mu: object = None

    def _blocks(self):
        return {k: getattr(self, k) for k in ("s", "y", "z", "mu") if getattr(self, k) is not None}

    def __add__(self, delta):
        """iterate + delta, block by block (a block absent on either side stays this side's): the tangent predictor
        problem.iterate() + problem.sensitivity_jvp(dp)."""
        if not isinstance(delta, Iterate):
            return NotImplemented

        def add(a, b):
            return a if b is None else b if a is None else np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64)

        mu = self.mu if not delta.mu else delta.mu if self.mu is None else self.mu + delta.mu
        return type(self)(x=add(self.x, delta.x), s=add(self.s, delta.s), y=add(self.y, delta.y), z=add(self.z, delta.z), mu=mu)


@dataclasses.dataclass
class Cotangent:
    """Cotangents on the whole end iterate and on the optimal cost, for Problem.sensitivity_vjp and
    Problem.sensitivity_batch_vjp: x (n), s (m_i), y (m_e), z (m_i) and cost (a number) — for a batch (B, n), (B, m_i),
    (B, m_e), (B, m_i) and (B).  None is absent; at least one must be given.  `cost` is the cost the solve reports: the
    cost of minimize(), the NEGATED objective of maximize()."""
    x: object = None
    s: object = None
    y: object = None
    z: object = None
    cost: object = None

    def _blocks(self):
        return {k: getattr(self, k) for k in ("x", "s", "y", "z", "cost") if getattr(self, k) is not None}


@dataclasses.dataclass
class Sensitivity:
    """What Problem.sensitivity() returns: the derivatives of the end iterate with respect to the parameters, in the
    user's units — dx (n_p, n), ds (n_p, m_i), dy (n_p, m_e), dz (n_p, m_i) — and `info`, a dict of
    slpx_sensitivity_info's members."""
    dx: np.ndarray
    ds: np.ndarray
    dy: np.ndarray
    dz: np.ndarray
    info: dict


@dataclasses.dataclass
class BatchIterate(Iterate):
    """Iterate for B instances: x (B, n), s and z (B, m_i), y (B, m_e), mu (B).  x is not read by solve_batch, whose
    initial_guesses are the instances' x."""


@dataclasses.dataclass
class BatchSensitivity:
    """What Problem.sensitivity_batch() returns: per instance the derivatives of its end iterate with respect to its
    parameter row — dx (B, n_p, n), ds (B, n_p, m_i), dy (B, n_p, m_e), dz (B, n_p, m_i) —, `status` (B: 0 computed,
    1 skipped, 2 not factored; rows of the latter two are NaN) and `info`, a list of B dicts of slpx_sensitivity_info's
    members."""
    dx: np.ndarray
    ds: np.ndarray
    dy: np.ndarray
    dz: np.ndarray
    status: np.ndarray
    info: list


@dataclasses.dataclass
class BatchResult:
    """What Problem.solve_batch returns: per instance the ExitStatus, the end iterate (x: (B, n),
    s, z: (B, m_i), y: (B, m_e)), the unscaled cost, the iteration and restoration counts; `report` holds
    the batch's totals and wall-clock phases.  How the batch ran: `rounds` lockstep Newton-step computations,
    `handoffs` instances handed to the batch-1 system for restoration, `driver` 0 none needed, 1 interior
    point, 2 SQP, 3 Newton.  `restoration_lockstep`: with restoration="lockstep", the instances restored in lockstep, the
    restoration phases, the lockstep rounds of the restoration loop and the instances that used the batch-1 system for a
    fallback (slpx_problem_batch_restoration_stats); all 0 with the hand-off."""
    status: list
    x: np.ndarray
    s: np.ndarray
    y: np.ndarray
    z: np.ndarray
    cost: np.ndarray
    iterations: np.ndarray
    restorations: np.ndarray
    report: dict
    rounds: int = 0
    handoffs: int = 0
    driver: int = 0
    restoration_lockstep: dict = dataclasses.field(default_factory=dict)
    # with solve_batch(warm_start=...) only: the end iterates in the user's units (s, y, z above are then in those units
    # too), and per instance the entries of the warm start its safeguard replaced or clamped
    iterate: object = None
    repaired: object = None


class Problem:
    """problem.hpp:66-720"""

    def __init__(self):
        self._p = _sa.Problem()
        self._decision_variables: list[Variable] = []
        self._pattern_cache = None
        self._cost = None  # (expression, sign) of minimize() / maximize()
        self.report = None  # counters and phase times of the last solve() that ran an iteration
        self.sensitivity_info = None  # slpx_sensitivity_info of the last sensitivity_jvp() / sensitivity_vjp()
        self.sensitivity_status = None  # per-instance status of the last batched sensitivity product

    # ---- model ----
    def decision_variable(self, rows=None, cols=1):
        """problem.hpp:78-104: no argument -> Variable, (rows[, cols]) -> VariableMatrix"""
        if rows is None:
            return self._new_variable()
        out = np.empty((int(rows), int(cols)), dtype=object)
        for r in range(out.shape[0]):
            for c in range(out.shape[1]):
                out[r, c] = self._new_variable()
        return VariableMatrix._of(out)

    def symmetric_decision_variable(self, rows):
        """problem.hpp:118-140: only the lower triangle is new variables"""
        out = np.empty((int(rows), int(rows)), dtype=object)
        for r in range(out.shape[0]):
            for c in range(r + 1):
                out[r, c] = out[c, r] = self._new_variable()
        return VariableMatrix._of(out)

    def _new_variable(self) -> Variable:
        self._pattern_cache = None
        v = Variable._wrap(self._p.decision_variable())
        self._decision_variables.append(v)
        return v

    def minimize(self, cost):
        self._pattern_cache = None
        self._cost = (Variable._lift(cost), 1.0)
        self._p.minimize(self._cost[0].node)

    def maximize(self, objective):
        self._pattern_cache = None
        self._cost = (Variable._lift(objective), -1.0)  # (stored, reported and differentiated negated)
        self._p.maximize(self._cost[0].node)

    def cost_value(self) -> float:
        """The cost at the variables' current values as a solve reports it: the cost of minimize(), the NEGATED objective
        of maximize(); 0 without either.  What cost_gradient() differentiates."""
        if self._cost is None:
            return 0.0
        return self._cost[1] * self._cost[0].value()

    def subject_to(self, constraint):
        self._pattern_cache = None
        if isinstance(constraint, EqualityConstraints):
            for c in constraint.constraints:
                self._p.subject_to_eq(c.node)
        elif isinstance(constraint, InequalityConstraints):
            for c in constraint.constraints:
                self._p.subject_to_ineq(c.node)
        else:
            raise TypeError("subject_to() takes EqualityConstraints or InequalityConstraints "
                            "(the result of ==, <=, >= or bounds())")

    def cost_function_type(self): return ExpressionType(self._p.types()[0])
    def equality_constraint_type(self): return ExpressionType(self._p.types()[1])
    def inequality_constraint_type(self): return ExpressionType(self._p.types()[2])

    # ---- solve ----
    def solve(self, **kwargs) -> ExitStatus:
        """problem.hpp:281-679.  Keyword arguments: tolerance, max_iterations, timeout,
        feasible_ipm, diagnostics, spy (bind_problem.cpp:80-112); anything else is a KeyError like
        the reference's."""
        allowed = {"tolerance", "max_iterations", "timeout", "feasible_ipm", "diagnostics", "spy", "warm_start"}
        for k in kwargs:
            if k not in allowed:
                raise KeyError(f"Invalid keyword argument: {k}")
        timeout = kwargs.pop("timeout", 0.0)
        if timeout is None or math.isinf(timeout):
            timeout = 0.0
        # warm_start = Iterate (no reference counterpart): the solve begins there; its x, where given, becomes the
        # variables' values first
        warm = kwargs.pop("warm_start", None)
        if warm is not None:
            if warm.x is not None:
                self._p.set_x(np.asarray(warm.x, dtype=np.float64).ravel())
            kwargs["warm_start"] = warm._blocks()
        # problem.hpp:304-313: nothing to do for a problem without cost and constraints
        if all(t <= ExpressionType.CONSTANT for t in self._p.types()):
            self.report = None
            return ExitStatus.SUCCESS
        status, self.report = self._p.solve(timeout=timeout, **kwargs)
        return ExitStatus(status)

    def iterate(self) -> "Iterate":
        """The primal-dual iterate the last solve() ended at, in the user's units (slpx_problem_get_iterate): pass it
        to the next solve(warm_start=...), of this problem after set_parameters() or of any with the same rows."""
        x, s, y, z, mu = self._p.iterate()
        return Iterate(x=x, s=s, y=y, z=z, mu=mu)

    def warm_start_repaired(self) -> int:
        """How many entries of its warm start the last solve's safeguard replaced or clamped."""
        return self._p.warm_start_repaired()

    def solve_batch(self, initial_guesses, **kwargs) -> "BatchResult":
        """B instances of this problem, one per row of `initial_guesses` (shape (B, n), decision-variable
        order), each solved as solve() would from that start, in one batched run on the device
        (slpx_problem_solve_batch).  Keyword arguments: tolerance, max_iterations, timeout, feasible_ipm
        (the timeout covers the whole batch); diagnostics and spy are accepted and ignored; restoration = "handoff"
        (default) or "lockstep": how instances that need feasibility restoration run it
        (slpx_problem_set_batch_restoration); parameters = array (B, n_p): instance b is this problem with row b for
        the values of parameters() (slpx_problem_solve_batch_parameters).  The variables' and the parameters'
        values are left as they are.  warm_start = BatchIterate (possibly empty): instance b begins at row b of its s,
        y, z and mu instead of the cold start — its x is not read, initial_guesses are the instances' x — and the
        result carries `iterate` (what the next call takes) and `repaired`, with s, y, z in the user's units
        (slpx_problem_solve_batch_warm).  Raises SlpxError where the library cannot run a batch (no device,
        callbacks registered)."""
        allowed = {"tolerance", "max_iterations", "timeout", "feasible_ipm", "diagnostics", "spy", "restoration",
                   "parameters", "warm_start"}
        for k in kwargs:
            if k not in allowed:
                raise KeyError(f"Invalid keyword argument: {k}")
        kwargs.pop("diagnostics", None)
        kwargs.pop("spy", None)
        timeout = kwargs.pop("timeout", 0.0)
        if timeout is None or math.isinf(timeout):
            timeout = 0.0
        guesses = np.asarray(initial_guesses, dtype=np.float64)
        n = len(self._decision_variables)
        if guesses.ndim != 2 or guesses.shape[1] != n or guesses.shape[0] < 1:
            raise ValueError(f"initial_guesses must have shape (B, {n}) with B >= 1")
        warm = kwargs.pop("warm_start", None)
        if warm is not None:
            kwargs["warm_start"] = warm._blocks()
        r = self._p.solve_batch(guesses, timeout=timeout, **kwargs)
        if warm is not None:
            return BatchResult(status=[ExitStatus(int(s)) for s in r["status"]], x=r["x"], s=r["s"], y=r["y"],
                               z=r["z"], cost=r["cost"], iterations=r["iterations"], restorations=r["restorations"],
                               report=r["report"], rounds=r["rounds"], handoffs=r["handoffs"], driver=r["driver"],
                               restoration_lockstep=r.get("restoration_lockstep", {}),
                               iterate=BatchIterate(x=r["x"], s=r["s"], y=r["y"], z=r["z"], mu=r["mu"]),
                               repaired=r["repaired"])
        return BatchResult(status=[ExitStatus(int(s)) for s in r["status"]], x=r["x"], s=r["s"], y=r["y"],
                           z=r["z"], cost=r["cost"], iterations=r["iterations"], restorations=r["restorations"],
                           report=r["report"], rounds=r["rounds"], handoffs=r["handoffs"], driver=r["driver"],
                           restoration_lockstep=r.get("restoration_lockstep", {}))

    def parameters(self) -> list:
        """The model's parameters: the free Variables that are not decision variables of this problem and that its cost
        or a constraint reaches, in the order of every parameter vector (ascending expression id).  Needs no device."""
        return [Variable._wrap(node) for node in self._p.parameters()]

    def set_parameters(self, values):
        """New values for parameters(), in that order, written in place into the compiled problem: the next solve() or
        solve_batch() does not compile again (Variable.set_value on a parameter does).  An MPC loop:

            problem.solve()
            for x_now in measurements:
                problem.set_parameters(x_now)
                problem.solve(warm_start=problem.iterate())
        """
        self._p.set_parameters(values)

    # ---- solution sensitivities (include/slpx.h): how iterate() moves with parameters(), in the user's units ----
    def sensitivity(self) -> "Sensitivity":
        """The Jacobian of the last solve's end iterate with respect to parameters(): dx (n_p, n), ds (n_p, m_i),
        dy (n_p, m_e), dz (n_p, m_i), row q the derivative with respect to parameter q, and `info` (what the call did:
        solves, factorizations, the inertia and regularization of what was factored, the largest backward error, the
        status of the solve the iterate came from).  n_p solves on one factorization."""
        r = self._p.sensitivity()
        return Sensitivity(dx=r["dx"], ds=r["ds"], dy=r["dy"], dz=r["dz"], info=r["info"])

    def sensitivity_jvp(self, dp) -> "Iterate":
        """The tangent of the end iterate along a parameter change dp (n_p), from one solve: an Iterate-shaped delta
        with mu = 0.  The predictor of an MPC loop:

            problem.solve()
            for p_now in measurements:
                it = problem.iterate() + problem.sensitivity_jvp(p_now - p_last)
                problem.set_parameters(p_now)
                problem.solve(warm_start=it)
        """
        r = self._p.sensitivity_jvp(dp)
        self.sensitivity_info = r["info"]
        return Iterate(x=r["dx"], s=r["ds"], y=r["dy"], z=r["dz"], mu=0.0)

    def sensitivity_vjp(self, v) -> np.ndarray:
        """(d x*/d p)^T v (n_p) for a cotangent v (n) on x: the gradient of l(x*(p)) with v = dl/dx, from ONE solve
        whatever n_p.  With a Cotangent instead of an array: the gradient of a loss on all of (x*, s*, y*, z*, cost*),
        sum_blocks (d block/dp)^T v_block + v_cost d cost*/dp, still from one solve."""
        if isinstance(v, Cotangent):
            grad, self.sensitivity_info = self._p.sensitivity_vjp_full(**v._blocks())
        else:
            grad, self.sensitivity_info = self._p.sensitivity_vjp(v)
        return grad

    def cost_gradient(self) -> np.ndarray:
        """d cost*/d p (n_p), the gradient of the optimal cost the last solve reported, from ONE solve instead of the n_p
        of sensitivity(): sensitivity_vjp(Cotangent(cost=1.0)).  For an interior-point model: of f at the barrier
        problem's solution, O(mu) from the model's."""
        return self.sensitivity_vjp(Cotangent(cost=1.0))

    # ---- batched sensitivities: functions of a BatchIterate and its parameter rows, not of the problem's state ----
    def sensitivity_batch(self, iterate, parameters) -> "BatchSensitivity":
        """The Jacobians of the B end iterates of a solve_batch(parameters=rows, warm_start=...) with respect to their own
        parameter rows: dx (B, n_p, n), ds (B, n_p, m_i), dy (B, n_p, m_e), dz (B, n_p, m_i), `status` (B: 0 computed,
        1 skipped — not finite or s <= 0 —, 2 not factored; rows of the latter two are NaN) and `info`, one dict per
        instance.  `iterate`: a BatchIterate, typically result.iterate.  n_p rounds of solves on one factorization."""
        r = self._p.sensitivity_batch(iterate, parameters)
        return BatchSensitivity(dx=r["dx"], ds=r["ds"], dy=r["dy"], dz=r["dz"], status=r["status"], info=r["info"])

    def sensitivity_batch_jvp(self, iterate, parameters, dp) -> "BatchIterate":
        """The tangents of the B end iterates along dp (B, n_p), one round of solves: a BatchIterate-shaped delta with
        mu = 0, so that result.iterate + it is the warm start of the next batch:

            r = problem.solve_batch(x0, parameters=rows, warm_start=BatchIterate())
            it = r.iterate + problem.sensitivity_batch_jvp(r.iterate, rows, rows_next - rows)
            r = problem.solve_batch(it.x, parameters=rows_next, warm_start=it)

        `sensitivity_status` (B) and `sensitivity_info` (B dicts) are those of this call."""
        r = self._p.sensitivity_batch_jvp(iterate, parameters, dp)
        self.sensitivity_status, self.sensitivity_info = r["status"], r["info"]
        return BatchIterate(x=r["dx"], s=r["ds"], y=r["dy"], z=r["dz"], mu=0.0)

    def sensitivity_batch_vjp(self, iterate, parameters, v) -> np.ndarray:
        """(d x*_b / d p_b)^T v_b (B, n_p) for cotangents v (B, n) on x, one round of solves whatever n_p.
        `sensitivity_status` and `sensitivity_info` are those of this call."""
        if isinstance(v, Cotangent):  # (rows per instance on any of x, s, y, z, cost)
            r = self._p.sensitivity_batch_vjp_full(iterate, parameters, **v._blocks())
        else:
            r = self._p.sensitivity_batch_vjp(iterate, parameters, v)
        self.sensitivity_status, self.sensitivity_info = r["status"], r["info"]
        return r["grad"]

    def cost_gradient_batch(self, iterate, parameters) -> np.ndarray:
        """d cost*_b / d p_b (B, n_p): sensitivity_batch_vjp with the cotangent 1 on every instance's cost alone."""
        B = np.shape(np.asarray(parameters))[0]
        return self.sensitivity_batch_vjp(iterate, parameters, Cotangent(cost=np.ones(B)))

    def sensitivity_batch_rhs(self, iterate, parameters) -> np.ndarray:
        """M (B, n_p, n + m_e + m_i): per instance and parameter r_x, r_e, r_i at its iterate; no factorization."""
        r = self._p.sensitivity_batch_rhs(iterate, parameters)
        self.sensitivity_status = r["status"]
        return r["M"]

    def restoration_steps_batch(self, x, s, y, z, mu, steps, **kwargs):
        """`steps` iterations of feasibility restoration from each of B iterates (rows of x, s, y, z; mu of length B), in
        lockstep on the device (slpx_problem_restoration_steps_batch).  Returns ([ExitStatus], x, s, y, z)."""
        status, x, s, y, z = self._p.restoration_steps_batch(x, s, y, z, mu, steps, **kwargs)
        return [ExitStatus(int(v)) for v in status], x, s, y, z

    def multistart(self, initial_guesses, **kwargs):
        """multistart.hpp:45-79 as one batched solve: every row of `initial_guesses` a start, then
        successful solves first, lowest cost among them.  Returns (status, cost, x) of that instance."""
        r = self.solve_batch(initial_guesses, **kwargs)
        best = min(range(len(r.status)), key=lambda b: (int(r.status[b] != ExitStatus.SUCCESS), r.cost[b]))
        return r.status[best], float(r.cost[best]), r.x[best].copy()

    def add_callback(self, callback):
        """problem.hpp:690-709: callback(info) -> True to stop (None counts as False)"""
        self._p.add_callback(lambda raw: bool(callback(IterationInfo(raw, self))))

    def clear_callbacks(self):
        self._p.clear_callbacks()

    # ---- helpers of IterationInfo ----
    def _patterns(self):
        if self._pattern_cache is None:
            s = self._p.system()
            self._pattern_cache = ({k: s.pattern(k) for k in range(5)}, s.info)
        return self._pattern_cache[0]

    def _value_count(self):
        self._patterns()
        return int(self._pattern_cache[1].get("nV", 0))

    def close(self):
        if self._p is not None:
            self._p.close()
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DynamicsType(enum.IntEnum):
    """ocp/dynamics_type.hpp:9-14"""
    EXPLICIT_ODE = 0
    DISCRETE = 1


class TimestepMethod(enum.IntEnum):
    """ocp/timestep_method.hpp:9-17"""
    FIXED = 0
    VARIABLE = 1
    VARIABLE_SINGLE = 2


class TranscriptionMethod(enum.IntEnum):
    """ocp/transcription_method.hpp:9-19"""
    DIRECT_TRANSCRIPTION = 0
    DIRECT_COLLOCATION = 1
    SINGLE_SHOOTING = 2


class OCP(Problem):
    """ocp.hpp:49-400 as the Python binding shows it (bind_ocp.cpp:29-128): dynamics is f(x, u)
    on column VariableMatrix arguments, dt a number of seconds."""

    def __init__(self, num_states, num_inputs, dt, num_steps, dynamics, dynamics_type=DynamicsType.EXPLICIT_ODE,
                 timestep_method=TimestepMethod.FIXED, transcription_method=TranscriptionMethod.DIRECT_TRANSCRIPTION):
        super().__init__()
        self._samples = int(num_steps) + 1
        self._f = dynamics
        self._kind = DynamicsType(dynamics_type)
        N1 = self._samples
        # one input more than there are steps: the last sample's constraints need one too (ocp.hpp:122-123)
        self._U = self.decision_variable(num_inputs, N1)
        if timestep_method == TimestepMethod.FIXED:
            self._DT = VariableMatrix(np.full((1, N1), float(dt)))
        elif timestep_method == TimestepMethod.VARIABLE_SINGLE:
            shared = self.decision_variable()
            shared.set_value(dt)
            self._DT = VariableMatrix._of(np.full((1, N1), shared, dtype=object))
        else:
            self._DT = self.decision_variable(1, N1)
            for k in range(N1):
                self._DT[0, k].set_value(dt)
        if transcription_method == TranscriptionMethod.SINGLE_SHOOTING:
            self._X = VariableMatrix(num_states, N1)  # expressions, filled by the rollout
        else:
            self._X = self.decision_variable(num_states, N1)
        if transcription_method == TranscriptionMethod.DIRECT_COLLOCATION and self._kind != DynamicsType.EXPLICIT_ODE:
            raise ValueError("OCP: direct collocation needs an explicit ODE")  # slp_assert at ocp.hpp:323

        for k in range(N1 - 1):
            h = self._DT[0, k]
            x0, u0 = self._X[:, k:k + 1], self._U[:, k:k + 1]
            if transcription_method == TranscriptionMethod.DIRECT_TRANSCRIPTION:  # ocp.hpp:359-379
                self.subject_to(self._X[:, k + 1:k + 2] == self._step(x0, u0, h))
            elif transcription_method == TranscriptionMethod.SINGLE_SHOOTING:  # ocp.hpp:382-401
                self._X[:, k + 1:k + 2] = self._step(x0, u0, h)
            else:  # ocp.hpp:322-357 (Hermite-Simpson)
                x1, u1 = self._X[:, k + 1:k + 2], self._U[:, k + 1:k + 2]
                f0, f1 = self._f(x0, u0), self._f(x1, u1)
                xdot_mid = (-3.0 / (2.0 * h)) * (x0 - x1) - 0.25 * (f0 + f1)
                x_mid = 0.5 * (x0 + x1) + (h / 8.0) * (f0 - f1)
                u_mid = 0.5 * (u0 + u1)
                self.subject_to(xdot_mid == self._f(x_mid, u_mid))

    def _step(self, x, u, h):
        """x_{k+1} as an expression of (x_k, u_k, h): the transition function itself, or one
        classical Runge-Kutta step of the ODE (ocp.hpp:310-319)"""
        if self._kind == DynamicsType.DISCRETE:
            return self._f(x, u)
        half = h * 0.5
        k1 = self._f(x, u)
        k2 = self._f(x + k1 * half, u)
        k3 = self._f(x + k2 * half, u)
        k4 = self._f(x + k3 * h, u)
        return x + (k1 + k2 * 2.0 + k3 * 2.0 + k4) * (h / 6.0)

    @staticmethod
    def _column(v, rows):
        if _is_scalar(v):
            return np.full((rows, 1), float(v))
        return v

    def constrain_initial_state(self, initial_state):
        self.subject_to(self.initial_state() == self._column(initial_state, self._X.rows()))

    def constrain_final_state(self, final_state):
        self.subject_to(self.final_state() == self._column(final_state, self._X.rows()))

    def for_each_step(self, callback):
        """ocp.hpp:183-213: callback(x, u) sees every sample, the last one included"""
        for k in range(self._samples):
            callback(self._X[:, k:k + 1], self._U[:, k:k + 1])

    def set_lower_input_bound(self, lower_bound):
        for k in range(self._samples):
            self.subject_to(self._U[:, k:k + 1] >= self._column(lower_bound, self._U.rows()))

    def set_upper_input_bound(self, upper_bound):
        for k in range(self._samples):
            self.subject_to(self._U[:, k:k + 1] <= self._column(upper_bound, self._U.rows()))

    def set_min_timestep(self, min_timestep):
        self.subject_to(self._DT >= float(min_timestep))

    def set_max_timestep(self, max_timestep):
        self.subject_to(self._DT <= float(max_timestep))

    def X(self): return self._X
    def U(self): return self._U
    def dt(self): return self._DT
    def initial_state(self): return self._X[:, 0:1]
    def final_state(self): return self._X[:, self._samples - 1:self._samples]


def multistart(solve, initial_guesses):
    """python/src/sleipnir/optimization/__init__.py:6-31 (multistart.hpp:45-79): every initial
    guess on its own thread — the expression graph of libslpx is per thread, so `solve` builds its
    problem inside the call like the reference's tests do — then successful solves first, lowest
    cost among them.  `solve(guess)` returns (status, cost, variables).  For many starts of ONE model,
    Problem.multistart / Problem.solve_batch solve them all in one batched run instead."""
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(initial_guesses)) as executor:
        futures = [executor.submit(solve, guess) for guess in initial_guesses]
        results = [f.result() for f in concurrent.futures.as_completed(futures)]
    return min(results, key=lambda r: (int(r[0] != ExitStatus.SUCCESS), r[1]))
