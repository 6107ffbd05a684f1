"""torch.autograd bindings of the batched kernels: skeleton_state(problem, theta) is Problem.skeleton_state with a backward
pass (mmx_eval_skeleton_state_backward), the counterpart of pymomentum/backend/triton_fk.py's _forward_kernel /
_backward_kernel pair.  Both directions are one kernel on the current stream; nothing goes through the host."""
from __future__ import annotations

import torch


class _SkeletonState(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, problem):
        ctx.problem = problem
        ctx.save_for_backward(theta)  # the backward kernel recomputes the forward kinematics from theta
        return problem.skeleton_state(theta)

    @staticmethod
    def backward(ctx, grad):
        (theta,) = ctx.saved_tensors
        return ctx.problem.skeleton_state_backward(theta, grad.contiguous()), None


def skeleton_state(problem, theta):
    """World transforms [B,J,8] = (tx,ty,tz, qx,qy,qz,qw, s) of theta [B,P] (float32, cuda, contiguous) on `problem`'s rig,
    differentiable with respect to theta.  Without theta.requires_grad (or under torch.no_grad()) this is
    problem.skeleton_state(theta): no graph node, no extra work."""
    if not (theta.requires_grad and torch.is_grad_enabled()):
        return problem.skeleton_state(theta)
    return _SkeletonState.apply(theta, problem)
