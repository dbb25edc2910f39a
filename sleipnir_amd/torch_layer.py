"""A solve as a differentiable torch operation: parameters in, x* out, the gradient through the solve from
Problem.sensitivity_vjp (include/slpx.h: solution sensitivities).  Imported on request only — nothing else in the package
needs torch.

    layer = SolveLayer(problem)                 # an optimization.Problem with parameters()
    p = torch.tensor([...], dtype=torch.float64, requires_grad=True)
    x = layer(p)                                # set_parameters(p); solve(); x*
    loss(x).backward()                          # p.grad = (dx*/dp)^T dloss/dx, one linear solve

Plumbing, like the rest of the package: the tensors are float64 on the CPU, the work happens in libslpx on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from sleipnir_amd import optimization

__all__ = ["SolveLayer"]


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
        return torch.from_numpy(np.array(layer.iterate.x, dtype=np.float64))

    @staticmethod
    def backward(ctx, grad_x):
        layer = ctx.layer
        if ctx.solve != layer.solves:
            raise RuntimeError("SolveLayer: backward of a forward that is not the layer's last (the sensitivities are those of "
                               "the last solve)")
        grad = layer.problem.sensitivity_vjp(grad_x.detach().cpu().to(torch.float64).numpy().ravel())
        return torch.from_numpy(np.array(grad, dtype=np.float64)).reshape(ctx.shape), None


class SolveLayer:
    """x*(p) of `problem` (an optimization.Problem) as a function of the values of problem.parameters().

    forward: set_parameters(p), solve(**solve_kwargs) — warm from the previous forward's iterate once there is one — and x*
    as a float64 CPU tensor; `status` is the ExitStatus of that solve and is not judged here.  backward: sensitivity_vjp,
    one linear solve on the KKT system at x*, valid for the layer's LAST forward only."""

    def __init__(self, problem: optimization.Problem, **solve_kwargs):
        self.problem = problem
        self.solve_kwargs = solve_kwargs
        self.iterate = None
        self.status = None
        self.solves = 0

    def __call__(self, parameters: torch.Tensor) -> torch.Tensor:
        return _Solve.apply(parameters, self)
