"""torch.autograd bindings of the batched kernels: skeleton_state(problem, theta) is Problem.skeleton_state with a backward
pass (mmx_eval_skeleton_state_backward), the counterpart of pymomentum/backend/triton_fk.py's _forward_kernel /
_backward_kernel pair; skin_points(skin, state) is Skin.skin_points with Skin.skin_points_backward, the counterpart of
triton_skinning.py's pair.  Each direction of each stage is one kernel on the current stream (the rest gradient, when asked
for, one more); nothing goes through the host.  The two compose: skin_points(skin, skeleton_state(problem, theta)).
vertex_normals(mesh, positions) is Mesh.vertex_normals with Mesh.vertex_normals_backward and takes the posed vertices of
skin_points, so that normal-dependent losses reach theta."""
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


class _SkinPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, rest, skin):
        ctx.skin = skin
        ctx.save_for_backward(state, rest if rest is not None else state.new_empty(0))
        ctx.has_rest = rest is not None
        return skin.skin_points(state, rest)

    @staticmethod
    def backward(ctx, grad):
        state, rest = ctx.saved_tensors
        want_rest = ctx.has_rest and ctx.needs_input_grad[1]
        state_grad, rest_grad = ctx.skin.skin_points_backward(state, grad.contiguous(), rest if ctx.has_rest else None, want_rest_grad=want_rest)
        return (state_grad if ctx.needs_input_grad[0] else None), rest_grad, None


def skin_points(skin, state, rest=None):
    """Posed vertices [B,V,3] of state [B,J,8] (float32, cuda, contiguous) on `skin` (capi.Skin), differentiable with respect
    to the state and to per-instance rest positions rest [B,V,3] when that is a tensor requiring grad.  Without an input that
    requires grad (or under torch.no_grad()) this is skin.skin_points(state, rest): no graph node, no extra work."""
    needs = state.requires_grad or (rest is not None and rest.requires_grad)
    if not (needs and torch.is_grad_enabled()):
        return skin.skin_points(state, rest)
    return _SkinPoints.apply(state.contiguous(), rest, skin)


class _VertexNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, positions, mesh):
        ctx.mesh = mesh
        normals, sums = mesh.vertex_normals(positions, want_sums=True)
        ctx.save_for_backward(positions, sums)  # the backward kernel reads the sums instead of recomputing a 2-ring
        return normals

    @staticmethod
    def backward(ctx, grad):
        positions, sums = ctx.saved_tensors
        return ctx.mesh.vertex_normals_backward(positions, sums, grad.contiguous()), None


def vertex_normals(mesh, positions):
    """Area-weighted vertex normals [B,V,3] of positions [B,V,3] (float32, cuda, contiguous) on `mesh` (capi.Mesh),
    differentiable with respect to the positions: one kernel forward, one backward (mmx_vertex_normals_backward, a gather
    without atomics).  Without positions.requires_grad (or under torch.no_grad()) this is mesh.vertex_normals(positions): no
    graph node, no sums buffer.  Composes with the other stages: vertex_normals(mesh, skin_points(skin, skeleton_state(...)))."""
    if not (positions.requires_grad and torch.is_grad_enabled()):
        return mesh.vertex_normals(positions)
    return _VertexNormals.apply(positions.contiguous(), mesh)
