"""Geometry queries on the device, with the call shapes of pymomentum.geometry.

find_closest_points is the nearest-point step of an ICP loop (mmx_closest_points: one kernel on the current stream), which
the reference runs on the CPU.  It composes with the mesh stages: the posed vertices of momentum_amd.autograd.skin_points go
in as points_source without leaving the device.  compute_vertex_normals (mmx_vertex_normals, differentiable) makes the
normals of those vertices that the overload with normals takes.  find_closest_points_on_mesh is the point-to-SURFACE form
(mmx_closest_points_on_mesh): the nearest point on the nearest triangle, with its face index and barycentric coordinates.
vertex_normal_equations (mmx_skin_normal_equations) turns such correspondences into the Gauss-Newton terms H = J^T J and
g = J^T r of the skinned mesh over the problem's parameters.
"""
from __future__ import annotations

import math

from . import capi

__all__ = ["find_closest_points", "find_closest_points_on_mesh", "compute_vertex_normals", "vertex_normal_equations"]


def compute_vertex_normals(vertex_positions, triangles):
    """Area-weighted vertex normals of a batch of posed meshes, the call shape of
    pymomentum.geometry.compute_vertex_normals(vertex_positions, triangles).

    vertex_positions [B, V, 3] (or [V, 3]: one element), a float32 cuda tensor; triangles a capi.Mesh, or an integer tensor /
    array [T, 3].  With a capi.Mesh this is the loop form: the handle's tables are on the device already and the call is one
    kernel.  With a tensor / array it is the convenience form: a handle is built for the call, which costs a host copy of the
    triangles, the incidence sort and an upload every time.

    A normal is the normalised sum of the face vectors (p_b - p_a) x (p_c - p_a) of the vertex's triangles (not normalised
    per face); a vertex of no triangle or of degenerate ones only gets zeros, a vertex next to a NaN position NaN.
    Differentiable with respect to vertex_positions (momentum_amd.autograd.vertex_normals); returns the shape it was given.
    """
    from . import autograd

    single = vertex_positions.dim() == 2
    pos = (vertex_positions[None] if single else vertex_positions).contiguous()
    assert pos.dim() == 3 and pos.shape[2] == 3, "vertex_positions must be [B, V, 3] or [V, 3]"
    own = not isinstance(triangles, capi.Mesh)
    mesh = capi.Mesh(triangles, int(pos.shape[1]), device=pos.device.index or 0) if own else triangles
    normals = autograd.vertex_normals(mesh, pos)
    # (a handle built here stays alive in the graph node until the backward pass has run; without a graph it goes now)
    return normals[0] if single else normals


def find_closest_points(*args, max_dist: float = math.inf, min_normal_dot: float = 0.0, **kwargs):
    """For every source point the nearest eligible target point of the same batch element.  Two forms, as in the reference:

        find_closest_points(points_source, points_target, max_dist=inf)
        find_closest_points(points_source, normals_source, points_target, normals_target, max_dist=inf, min_normal_dot=0.0)

    points_source [B, N, 3] (or [N, 3]: one element), points_target [B, M, 3] or [M, 3] (shared by the batch), float32 cuda
    tensors; the normals are laid out like their points and used as given (not renormalised).  A target is eligible when its
    squared distance (differences first, in float32) is finite and <= max_dist^2 and, with normals,
    n_source . n_target >= min_normal_dot; among equally near targets the lowest index wins; a NaN anywhere in a pair makes
    the pair ineligible.  (The reference's name and default for the normal threshold are still to be confirmed: see the
    PROVENANCE note in include/mmx.h.)

    Returns (closest_points [B, N, 3] float32, zeros where invalid; index [B, N] int32, -1 where invalid; valid [B, N] bool).

    The results carry no autograd graph.  Where a gradient to the target (or a differentiable distance) is wanted, gather in
    torch: `target[b, index.long()]` on the valid rows, and take the distance to the source from that.
    """
    import torch

    names2, names4 = ("points_source", "points_target"), ("points_source", "normals_source", "points_target", "normals_target")
    tensors = [a for a in args if isinstance(a, torch.Tensor)]
    rest = list(args[len(tensors) :])
    with_normals = len(tensors) == 4 or "normals_source" in kwargs or "normals_target" in kwargs
    names = names4 if with_normals else names2
    given = dict(zip(names, tensors))
    for k in names:
        if k in kwargs:
            assert k not in given, f"{k} given twice"
            given[k] = kwargs.pop(k)
    assert len(tensors) <= len(names) and set(given) == set(names), f"find_closest_points takes {names}"
    if rest:
        max_dist = rest.pop(0)
    if rest and with_normals:
        min_normal_dot = rest.pop(0)
    assert not rest and not kwargs, "unexpected arguments"
    src, tgt = given["points_source"], given["points_target"]
    ns, nt = given.get("normals_source"), given.get("normals_target")
    single = src.dim() == 2
    prep = lambda t, lift: None if t is None else (t.detach()[None] if lift else t.detach()).contiguous()
    index, _, points = capi.closest_points(
        prep(src, single), prep(tgt, False), float(max_dist), prep(ns, single), prep(nt, False), float(min_normal_dot), want_dist2=False, want_points=True
    )  # fmt: skip
    valid = index >= 0
    if single:
        return points[0], index[0], valid[0]
    return points, index, valid


def find_closest_points_on_mesh(points_source, vertices_target, faces_target, *, max_dist: float = math.inf):
    """For every source point the nearest point ON the posed triangle mesh of the same batch element, the call shape of
    pymomentum.geometry.find_closest_points_on_mesh(points_source, vertices_target, faces_target).

    points_source [B, N, 3] (or [N, 3]: one element; vertices_target is then [V, 3]), vertices_target [B, V, 3] or [V, 3]
    (shared by the batch), float32 cuda tensors; faces_target a capi.Mesh (the loop form: the handle's triangle list is on
    the device already and the call is one kernel) or an integer tensor / array [T, 3] (the convenience form: a handle is
    built for the call).  max_dist is an extension of this library (keyword-only; inf reproduces a call without it).

    A triangle with a repeated vertex (a face vector of exact zeros) or a non-finite vertex is never returned; among equally
    near triangles the lowest face index wins; a non-finite source is invalid.  See include/mmx.h for the arithmetic.

    Returns (valid [B, N] bool; closest_points [B, N, 3] float32, zeros where invalid; face_index [B, N] int32, -1 where
    invalid; barycentric [B, N, 3] float32 = the weights of the face's corners in the face's own order, each >= 0, zeros
    where invalid).

    The results carry no autograd graph.  The differentiable closest point is the recombination in torch, on the valid rows
    (faces the [T, 3] long tensor of the mesh, b the batch index of a row):

        (barycentric[..., None] * vertices[b, faces[face_index]]).sum(-2)

    whose gradient reaches all three vertices of each face (the weights are held fixed, as in point-to-plane ICP).
    """
    single = points_source.dim() == 2
    src = (points_source.detach()[None] if single else points_source.detach()).contiguous()
    vtx = vertices_target.detach().contiguous()
    assert src.dim() == 3 and src.shape[2] == 3, "points_source must be [B, N, 3] or [N, 3]"
    assert vtx.dim() in (2, 3) and vtx.shape[-1] == 3, "vertices_target must be [B, V, 3] or [V, 3]"
    own = not isinstance(faces_target, capi.Mesh)
    mesh = capi.Mesh(faces_target, int(vtx.shape[-2]), device=src.device.index or 0) if own else faces_target
    try:
        face, bary, points, _ = mesh.closest_points(src, vtx, float(max_dist), want_barycentric=True, want_points=True, want_dist2=False)
    finally:
        if own:
            import torch

            torch.cuda.current_stream(src.device).synchronize()  # (the kernel reads the handle's triangle list)
            mesh.close()
    valid = face >= 0
    if single:
        return valid[0], points[0], face[0], bary[0]
    return valid, points, face, bary


def vertex_normal_equations(
    problem, skin, theta, target, *, vertex=None, barycentric=None, normal=None, weight=None, rest=None, function_weight=1.0,
    want=("jtj", "jtr", "err"), parts=1, workspace=None,
):
    """Gauss-Newton terms of vertex constraints on a skinned mesh: capi.Problem.vertex_normal_equations with the outputs of
    the closest-point queries taken as they come.

    problem a capi.Problem, skin a capi.Skin on its rig, theta [B, P]; target [B, C, 3] the points the constrained mesh points
    are pulled to.  vertex: None (constraint c is vertex c), vertex indices [B, C], or corner triples [B, C, 3] -- e.g.
    faces[face_index.long()] of find_closest_points_on_mesh, whose -1 rows may stay as they are: an index outside [0, V) in
    any corner skips the constraint -- with barycentric [B, C, 3].  normal [B, C, 3]: point-to-plane rows n . (x - target), the
    normal used as given.  weight [B, C]: floats, or a bool mask such as `valid` (False = skipped).

    Returns (jtj [B, n, n], jtr [B, n], err [B] float64) over the enabled parameters, in the layout of
    problem.normal_equations: the two sets of terms add.  The results carry no autograd graph.

    parts and workspace go to capi.Problem.vertex_normal_equations as they are: parts > 1 (or "auto") divides every instance
    over several workgroups -- for one scan or a short clip against a dense mesh; an instance's bits depend on its inputs and
    the effective parts only, and "auto" depends on the batch size.
    """
    import torch

    prep = lambda t: None if t is None else t.detach()
    if vertex is not None and vertex.dtype != torch.int32:
        vertex = vertex.to(torch.int32)
    if weight is not None and weight.dtype != torch.float32:
        weight = weight.to(torch.float32)
    return problem.vertex_normal_equations(
        skin, theta.detach().contiguous(), prep(target), vertex=prep(vertex), barycentric=prep(barycentric), normal=prep(normal),
        weight=prep(weight), rest=prep(rest), function_weight=function_weight, want=want, parts=parts, workspace=workspace,
    )  # fmt: skip
