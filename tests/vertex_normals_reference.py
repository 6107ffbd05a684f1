"""Reference of the area-weighted vertex normals (mmx_vertex_normals / mmx_vertex_normals_backward): the gather / cross /
index_add / normalise a caller writes in torch, parameterised by dtype and differentiable by torch autograd.  Checked on its
own in tests/test_vertex_normals_reference.py.

    c_t = (p_b - p_a) x (p_c - p_a)        m_v = sum of c_t over the triangles of v (once per corner)        n_v = m_v / |m_v|

and n_v = 0 where m_v = 0 (a vertex of no triangle, or of degenerate ones only).  Face vectors are not normalised.

MESHES are the parity shapes of tests/test_gpu_vertex_normals.py.  Their condition of admission (held by
tests/test_vertex_normals_reference.py on the CPU, for every one of them, with the cotangent of parity_case): the float32
reference stays within 1e-6 of the float64 reference, for the normals, the sums and the position gradient, in the distance
max|x - x64| / max|x64| per instance.
The GPU test's bound is 4 x that float32 distance, so a mesh on which float32 itself is lost would make the bound meaningless.
"""
import numpy as np
import torch

from momentum_amd import make_test_mesh

CAP = 1e-6  # the float32 reference's largest admissible distance from the float64 reference on a parity mesh


def vertex_normals(positions, triangles, want_sums=False):
    """positions [B, V, 3] (any float dtype / device), triangles [T, 3] int64 on the same device -> normals [B, V, 3]
    (and the unnormalised sums)."""
    a, b, c = (positions[:, triangles[:, k]] for k in range(3))  # [B, T, 3]
    face = torch.cross(b - a, c - a, dim=-1)
    sums = torch.zeros_like(positions)
    for k in range(3):
        sums = sums.index_add(1, triangles[:, k], face)
    s = (sums * sums).sum(-1, keepdim=True)
    on = s > 0
    normals = torch.where(on, sums / torch.sqrt(torch.where(on, s, torch.ones_like(s))), torch.zeros_like(sums))
    return (normals, sums) if want_sums else normals


def vjp_autograd(positions, triangles, cot, dtype, device="cpu"):
    """dict(normals, sums, position_grad = d sum(cot * normals) / d positions) by torch autograd in `dtype`, as numpy."""
    p = torch.as_tensor(np.asarray(positions), dtype=dtype, device=device).clone().requires_grad_(True)
    tri = torch.as_tensor(np.asarray(triangles, np.int64), device=device)
    normals, sums = vertex_normals(p, tri, want_sums=True)
    (normals * torch.as_tensor(np.asarray(cot), dtype=dtype, device=device)).sum().backward()
    return dict(normals=normals.detach().cpu().numpy(), sums=sums.detach().cpu().numpy(), position_grad=p.grad.cpu().numpy())


def vjp_np(positions, triangles, cot):
    """One instance in float64, the formulas of include/mmx.h written as loops: h_v = (g_v - n_v (n_v . g_v)) / |m_v|,
    H_t = h_a + h_b + h_c, grad_x = sum over (t, corner of x) of (p_next - p_prev) x H_t.  -> (normals, sums, grad)."""
    p, g, tri = np.asarray(positions, np.float64), np.asarray(cot, np.float64), np.asarray(triangles)
    m = np.zeros_like(p)
    for a, b, c in tri:
        f = np.cross(p[b] - p[a], p[c] - p[a])
        m[a] += f
        m[b] += f
        m[c] += f
    n, h = np.zeros_like(p), np.zeros_like(p)
    for v in range(len(p)):
        s = m[v] @ m[v]
        if s > 0:
            n[v] = m[v] / np.sqrt(s)
            h[v] = (g[v] - n[v] * (n[v] @ g[v])) / np.sqrt(s)
    grad = np.zeros_like(p)
    for t in tri:
        H = h[t[0]] + h[t[1]] + h[t[2]]
        for k in range(3):
            grad[t[k]] += np.cross(p[t[(k + 1) % 3]] - p[t[(k + 2) % 3]], H)
    return n, m, grad


def dist(x, x64):
    """max|x - x64| / max|x64| per instance: [B]."""
    x, x64 = np.asarray(x, np.float64).reshape(len(x), -1), np.asarray(x64, np.float64).reshape(len(x64), -1)
    scale = np.abs(x64).max(axis=1)
    return np.abs(x - x64).max(axis=1) / np.where(scale > 0, scale, 1.0)


def rings(triangles, num_vertices, v):
    """(closed 1-ring, closed 2-ring) of vertex v as boolean masks [V]."""
    tri = np.asarray(triangles)
    one = np.zeros(num_vertices, bool)
    one[v] = True
    one[tri[(tri == v).any(axis=1)].reshape(-1)] = True
    two = one.copy()
    two[tri[one[tri].any(axis=1)].reshape(-1)] = True
    return one, two


# ---- the parity meshes: name -> (positions [B, V, 3] float32, triangles [T, 3] int32)
WORKGROUP = 256  # kMeshThreads: vertices of one instance a workgroup of either kernel takes (momentum_amd/csrc/mmx_mesh_tables.hpp)


def instances(positions, B, seed, jitter):
    """[B, V, 3] float32: B jittered copies of positions [V, 3] (the mesh's pose differs per instance)."""
    rng = np.random.default_rng(seed)
    return (np.asarray(positions, np.float64)[None] + jitter * rng.uniform(-1.0, 1.0, size=(B,) + positions.shape)).astype(np.float32)


def torus(nu, nv, B, seed, isolated=0, offset=(0.0, 0.0, 0.0), noise=0.12):
    """The make_test_mesh torus with `isolated` vertices of no triangle appended, as B instances (each jittered by a further
    2 % of the shortest grid edge)."""
    m = make_test_mesh(nu, nv, noise, seed, offset)
    pos = m.positions
    if isolated:
        extra = np.random.default_rng(seed + 1).uniform(-0.4, 0.4, size=(isolated, 3)) + np.asarray(offset)
        pos = np.concatenate([pos, extra.astype(np.float32)])
    clean = make_test_mesh(nu, nv, 0.0, seed).positions
    edge = np.linalg.norm(clean[1] - clean[0])  # (a minor-circle edge; the scale of the per-instance jitter only)
    return instances(pos, B, seed + 2, 0.02 * edge), m.triangles


def fan(valence, B, seed, turns=100):
    """An open fan wound `turns` times around its hub: hub 0 of the given valence, rim vertices 1 .. valence + 1 on a helix of
    radius 0.3 around it that climbs from z = -0.3 to 0.3, triangles (0, i, i + 1).  Winding keeps the apex angle at
    2 pi turns / valence (36 degrees) -- a flat fan of valence 1000 is made of slivers, on which float32 itself loses the
    normal (the float32 reference then misses the cap by a factor of 3 to 9)."""
    i = np.arange(valence + 1)
    th = 2.0 * np.pi * turns * i / valence
    rim_edge = 0.3 * 2.0 * np.sin(np.pi * turns / valence)
    rng = np.random.default_rng(seed)
    pos = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([0.3 * np.cos(th), 0.3 * np.sin(th), -0.3 + 0.6 * i / valence], axis=1)])
    pos += 0.1 * rim_edge * rng.uniform(-1.0, 1.0, size=pos.shape)
    tri = np.stack([np.zeros(valence, np.int64), 1 + i[:-1], 2 + i[:-1]], axis=1).astype(np.int32)
    return instances(pos.astype(np.float32), B, seed + 2, 0.02 * rim_edge), tri


MESHES = {
    "single_triangle": lambda: (instances(np.array([[0.1, 0.2, -0.3], [0.9, 0.1, 0.2], [0.3, 0.8, 0.4]], np.float32), 2, 5, 0.05), np.array([[0, 1, 2]], np.int32)),
    "torus_8x4_b1": lambda: torus(8, 4, 1, 11),
    "torus_8x4_b5": lambda: torus(8, 4, 5, 11),
    "fan_1000": lambda: fan(1000, 2, 21),  # the heavy vertex: one lane walks 1000 entries
    "torus_64x32_offset": lambda: torus(64, 32, 3, 31, offset=(1.0, 1.5, -0.5)),  # V = 2048, away from the origin
}
for _v in (63, 64, 65):  # a partial last wave: 10 x 6 = 60 grid vertices and isolated ones
    MESHES[f"edge_v{_v}"] = lambda v=_v: torus(10, 6, 2, 40 + v, isolated=v - 60)
for _v in (WORKGROUP - 1, WORKGROUP, WORKGROUP + 1):  # a partial last workgroup: 21 x 12 = 252 grid vertices and isolated ones
    MESHES[f"edge_v{_v}"] = lambda v=_v: torus(21, 12, 2, 50 + v, isolated=v - 252)


def cotangent(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def parity_case(name):
    """(positions [B, V, 3], triangles [T, 3], cotangent [B, V, 3]) of a parity mesh: the inputs the condition of admission is
    held on are the inputs the GPU test runs."""
    pos, tri = MESHES[name]()
    return pos, tri, cotangent(pos.shape, 7)
