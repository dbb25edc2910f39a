"""A solve as a differentiable torch operation: parameters in, x* out — or any of x*, s*, y*, z* and the optimal cost
(outputs=...) —, the gradient through the solve from Problem.sensitivity_vjp (include/slpx.h: solution sensitivities, the
full vjp).  Imported on request only — nothing else in the package needs torch.

    layer = SolveLayer(problem)                 # an optimization.Problem with parameters()
    p = torch.tensor([...], dtype=torch.float64, requires_grad=True)
    x = layer(p)                                # set_parameters(p); solve(); x*
    loss(x).backward()                          # p.grad = (dx*/dp)^T dloss/dx, one linear solve

    layer = BatchSolveLayer(problem)            # a minibatch: rows (B, n_p) in, x* (B, n) out
    x = layer(rows)                             # one solve_batch(parameters=rows), warm from the last forward
    loss(x).backward()                          # rows.grad from ONE sensitivity_batch_vjp

    layer = SolveLayer(problem, outputs=("x", "y", "cost"))
    x, y, cost = layer(p)                       # a tuple, in the order x, s, y, z, cost
    loss(x, y, cost).backward()                 # every incoming gradient goes into ONE vjp: still one linear solve

Plumbing, like the rest of the package: the tensors are float64 on the CPU, the work happens in libslpx on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from sleipnir_amd import optimization

__all__ = ["SolveLayer", "BatchSolveLayer", "OUTPUTS"]

OUTPUTS = ("x", "s", "y", "z", "cost")


def _check_outputs(outputs, who):
    outputs = tuple(outputs)
    if not outputs or any(k not in OUTPUTS for k in outputs) or list(outputs) != [k for k in OUTPUTS if k in outputs]:
        raise ValueError(f"{who}: outputs must be a non-empty subset of {OUTPUTS}, in that order")
    return outputs


def _cotangent(outputs, grads):
    """the incoming gradients that are not None as an optimization.Cotangent (None: none of them is there)"""
    blocks = {k: g.detach().cpu().to(torch.float64).numpy() for k, g in zip(outputs, grads) if g is not None}
    return optimization.Cotangent(**blocks) if blocks else None


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, parameters, layer):
        if parameters.dtype != torch.float64 or parameters.device.type != "cpu":
            raise TypeError("SolveLayer: the parameters must be a float64 tensor on the CPU")
        problem = layer.problem
        problem.set_parameters(parameters.detach().numpy().ravel())
        # warm from the iterate the previous forward ended at, once there is one
        kwargs = dict(layer.solve_kwargs)
        if layer.iterate is not None:
            kwargs["warm_start"] = layer.iterate
        layer.status = problem.solve(**kwargs)
        layer.iterate = problem.iterate()
        layer.solves += 1
        ctx.layer, ctx.solve, ctx.shape = layer, layer.solves, parameters.shape
        if layer.outputs == ("x",):
            return torch.from_numpy(np.array(layer.iterate.x, dtype=np.float64))
        ctx.set_materialize_grads(False)
        layer.cost = problem.cost_value()
        values = {"x": layer.iterate.x, "s": layer.iterate.s, "y": layer.iterate.y, "z": layer.iterate.z, "cost": layer.cost}
        return tuple(torch.from_numpy(np.array(values[k], dtype=np.float64)) for k in layer.outputs)

    @staticmethod
    def backward(ctx, *grads):
        layer = ctx.layer
        if ctx.solve != layer.solves:
            raise RuntimeError("SolveLayer: backward of a forward that is not the layer's last (the sensitivities are those of "
                               "the last solve)")
        if layer.outputs == ("x",):
            grad = layer.problem.sensitivity_vjp(grads[0].detach().cpu().to(torch.float64).numpy().ravel())
        else:
            v = _cotangent(layer.outputs, grads)
            if v is None:
                return None, None
            grad = layer.problem.sensitivity_vjp(v)
        return torch.from_numpy(np.array(grad, dtype=np.float64)).reshape(ctx.shape), None


class SolveLayer:
    """x*(p) of `problem` (an optimization.Problem) as a function of the values of problem.parameters().

    forward: set_parameters(p), solve(**solve_kwargs) — warm from the previous forward's iterate once there is one — and x*
    as a float64 CPU tensor; `status` is the ExitStatus of that solve and is not judged here.  backward: sensitivity_vjp,
    one linear solve on the KKT system at x*, valid for the layer's LAST forward only.

    outputs: a non-empty subset of ("x", "s", "y", "z", "cost"), in that order — the end iterate's blocks in the user's
    units and the cost the solve reports (`cost`).  The default returns the one tensor x*; anything else a tuple, and
    backward hands every incoming gradient that is not None to ONE sensitivity_vjp(Cotangent(...))."""

    def __init__(self, problem: optimization.Problem, outputs=("x",), **solve_kwargs):
        self.problem = problem
        self.outputs = _check_outputs(outputs, "SolveLayer")
        self.cost = None
        self.solve_kwargs = solve_kwargs
        self.iterate = None
        self.status = None
        self.solves = 0

    def __call__(self, parameters: torch.Tensor):
        return _Solve.apply(parameters, self)


class _BatchSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, parameters, layer):
        if parameters.dtype != torch.float64 or parameters.device.type != "cpu" or parameters.dim() != 2:
            raise TypeError("BatchSolveLayer: the parameters must be a float64 tensor (B, n_p) on the CPU")
        problem = layer.problem
        rows = np.ascontiguousarray(parameters.detach().numpy())
        B = rows.shape[0]
        # warm from the iterates the previous forward ended at while the batch size stays; else from x0, duals cold
        if layer.iterate is not None and np.shape(layer.iterate.x)[0] == B:
            guesses, warm = layer.iterate.x, layer.iterate
            layer.warm_forwards += 1
        else:
            n = len(problem._decision_variables)
            x0 = problem._p.get_x() if layer.x0 is None else np.asarray(layer.x0, dtype=np.float64)
            guesses, warm = np.ascontiguousarray(np.broadcast_to(x0, (B, n))), optimization.BatchIterate()
        result = problem.solve_batch(guesses, parameters=rows, warm_start=warm, **layer.solve_kwargs)
        layer.status, layer.iterate, layer.rows = result.status, result.iterate, rows.copy()
        layer.solves += 1
        ctx.layer, ctx.solve = layer, layer.solves
        if layer.outputs == ("x",):
            return torch.from_numpy(np.array(result.iterate.x, dtype=np.float64))
        ctx.set_materialize_grads(False)
        layer.cost = np.array(result.cost, dtype=np.float64)
        values = {"x": result.iterate.x, "s": result.iterate.s, "y": result.iterate.y, "z": result.iterate.z, "cost": layer.cost}
        return tuple(torch.from_numpy(np.array(values[k], dtype=np.float64)) for k in layer.outputs)

    @staticmethod
    def backward(ctx, *grads):
        layer = ctx.layer
        if ctx.solve != layer.solves:
            raise RuntimeError("BatchSolveLayer: backward of a forward that is not the layer's last (the sensitivities are "
                               "those of the last batch)")
        if layer.outputs == ("x",):
            v = grads[0].detach().cpu().to(torch.float64).numpy()
        else:
            v = _cotangent(layer.outputs, grads)
            if v is None:
                return None, None
        grad = layer.problem.sensitivity_batch_vjp(layer.iterate, layer.rows, v)
        layer.sensitivity_status = np.array(layer.problem.sensitivity_status)
        grad = np.where((layer.sensitivity_status != 0)[:, None], 0.0, grad)
        return torch.from_numpy(np.ascontiguousarray(grad, dtype=np.float64)), None


class BatchSolveLayer:
    """x*_b(p_b) for a minibatch of parameter rows of `problem` (an optimization.Problem) in one solve_batch.

    forward: a float64 CPU tensor (B, n_p) -> solve_batch(parameters=rows, warm_start=...), warm from the previous forward's
    iterates while B is unchanged (else from x0 — (n) or (B, n); None: the variables' values — with the duals cold), and
    x* (B, n); `status` holds the instances' ExitStatus and is not judged here.  backward: ONE sensitivity_batch_vjp, valid
    for the layer's LAST forward only; an instance that could not be differentiated (`sensitivity_status` != 0) gets a
    zero gradient row.

    outputs: as SolveLayer's, per instance — x (B, n), s and z (B, m_i), y (B, m_e), cost (B); the default returns the one
    tensor x*, anything else a tuple whose incoming gradients go into ONE sensitivity_batch_vjp(Cotangent(...))."""

    def __init__(self, problem: optimization.Problem, x0=None, outputs=("x",), **solve_kwargs):
        self.problem = problem
        self.outputs = _check_outputs(outputs, "BatchSolveLayer")
        self.cost = None
        self.x0 = x0
        self.solve_kwargs = solve_kwargs
        self.iterate = None
        self.rows = None
        self.status = None
        self.sensitivity_status = None
        self.solves = 0
        self.warm_forwards = 0  # forwards that began at the previous forward's iterates

    def __call__(self, parameters: torch.Tensor):
        return _BatchSolve.apply(parameters, self)
