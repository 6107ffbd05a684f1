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

ENTRY_MESHES, further down, are the meshes of tests/test_gpu_vertex_normals_entries.py, which holds every entry to a rule of its
own (forward_rule, backward_rule) and so needs no such condition: uneven lists, folds, centimetres, degenerate triangles.
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


# ---- entry by entry (tests/test_gpu_vertex_normals_entries.py; shown sound and with teeth in tests/test_vertex_normals_reference.py)
"""The per-entry rules.  u = 2^-24, e = 2^-52; positions are float32 taken exactly into float64; vertex v has n_v entries
(triangle, corner).  absface_t is the cross product of e1 = p_b - p_a and e2 = p_c - p_a written on absolute values (x:
|e1y||e2z| + |e1z||e2y|, cyclically), A_v its sum over v's entries, eps_v = (n_v + 8) e A_v.

    sums            |x - x64| <= u |x64| + eps_v
    normals         |x_k - n_k| <= u |n_k| + (eps_k + |n_k| sum_j |n_j| eps_j) / M + 4 e |n_k|        M = |m64_v| > 0
    position_grad   |x - x64| <= u |x64| + (n_v + 16) e S_v

every bound + 2^-149 (float32's subnormal spacing).  x64 of the gradient is the header's formula in float64 on the FLOAT32 SUMS
THE KERNEL IS GIVEN (backward_from_sums64), not autograd through a forward.  Habs_k = (s |g_k| + |m_k| sum_j |m_j g_j|) / (s sqrt s)
per vertex (0 for s = 0), Habs_t its sum over the three corners, S_v the sum over v's entries of the absolute-value cross product
of |p_next - p_prev| with Habs_t.  Where A or S is 0 the rule asks for an exact zero; so it does for the normals where M = 0
(with A > 0 that is a vertex of repeated-corner triangles, or of triangles each followed by its reversed copy: every order
sums to exact zeros).  A vertex with no entry gets positive zeros.  No entry is left out.

The constants count roundings, each of 2^-53 = e / 2 relative to the absolute-value term it acts on; kernel and float64
reference are counted alike, so every count below is taken twice and halved -- it is the count in units of e.
  8   per face vector: two differences (1 each on their factor: 2 on a product), a product (1), the subtraction (1) = 4; the
      sum of n terms n - 1; the conversion of the reference's own order; together n + 3 <= n + 8 with 5 in hand for the
      second-order terms of lists of a few hundred entries.
  4   s = |m|^2 (3 on a sum of squares: 1.5 on its root), the root (1), the reciprocal or division (1), the product (1): 4.5
      roundings of e / 2 for each of the two sides: 4.5 e <= 4 e + what the first-order term of eps leaves.
  16  h: s (3) and m . g (3, on sum |m_j g_j|), the products s g and m (m . g) (1 each), their difference (1), s sqrt s (1.5 x 3 for
      s, 1 root, 1 product), the division (1): at most 13 on Habs; H_t = (h_a + h_b) + h_c (2); the difference p_next - p_prev
      (1); the cross product (2); the sum of n terms n - 1: n + 17 roundings of e / 2 a side, (n + 17) e / 2 x 2 sides with
      the reference's h written as (g - n (n . g)) / |m| (12 on Habs): <= (n + 16) e.
They are derived, not measured."""
from momentum_amd import capi  # noqa: E402

U32, E64, TINY = 2.0**-24, 2.0**-52, 2.0**-149
KEYS = ("normals", "sums", "position_grad")


def _cross(u, v):
    """Both products rounded, then the difference (faceVector's cross: never an fma)."""
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _abscross(u, v):
    u, v = np.abs(u), np.abs(v)
    return np.stack([u[..., 1] * v[..., 2] + u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] + u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] + u[..., 1] * v[..., 0]], -1)


def _cross_fused(u, v):
    """The planted fault: u.y v.z - u.z v.y contracted into fma(u.y, v.z, -(u.z v.y)), exactly (rational arithmetic, one
    rounding)."""
    from fractions import Fraction

    def fms(a, b, c, d):
        cd = c * d
        out = np.empty_like(cd)
        for i, (x, y, z) in enumerate(zip(a.ravel().tolist(), b.ravel().tolist(), cd.ravel().tolist())):
            out.flat[i] = float(Fraction(x) * Fraction(y) - Fraction(z))
        return out

    return np.stack([fms(u[..., 1], v[..., 2], u[..., 2], v[..., 1]), fms(u[..., 2], v[..., 0], u[..., 0], v[..., 2]), fms(u[..., 0], v[..., 1], u[..., 1], v[..., 0])], -1)


def incidence(triangles, num_vertices):
    """capi.host_mesh_tables as int64: (vertex_start [V + 1], n_v [V], entry_triangle [E], entry_corner [E])."""
    t = capi.host_mesh_tables(num_vertices, triangles)
    start = t["vertex_start"].astype(np.int64)
    return start, np.diff(start), t["entry_triangle"].astype(np.int64), t["entry_corner"].astype(np.int64)


def _scatter(values, tri, V):
    """sum over the corners k of values[k] [B, T, 3] into [B, V, 3]: triangle after triangle, corner 0 of all first."""
    out = np.zeros((values[0].shape[0], V, 3))
    for k in range(3):
        np.add.at(out, (slice(None), tri[:, k]), values[k])
    return out


def forward64(positions, triangles):
    """(normals, sums) [B, V, 3] in float64 from float32 positions: numpy, scattered triangle by triangle (not the kernels'
    order); zeros where the sum is zero."""
    p, tri = np.asarray(positions, np.float64), np.asarray(triangles, np.int64)
    a, b, c = (p[:, tri[:, k]] for k in range(3))
    face = _cross(b - a, c - a)
    sums = _scatter([face] * 3, tri, p.shape[1])
    M = np.sqrt((sums * sums).sum(-1, keepdims=True))
    return np.where(M > 0, sums / np.where(M > 0, M, 1.0), 0.0), sums


def _h64(sums, cot):
    m, g = np.asarray(sums, np.float64), np.asarray(cot, np.float64)
    M = np.sqrt((m * m).sum(-1, keepdims=True))
    on = M > 0
    n = m / np.where(on, M, 1.0)
    return np.where(on, (g - n * (n * g).sum(-1, keepdims=True)) / np.where(on, M, 1.0), 0.0)


def backward_from_sums64(positions, triangles, sums, cot):
    """position_grad [B, V, 3] in float64 by the formulas of include/mmx.h from the sums GIVEN (the float32 ones the kernel
    reads, or any others): h_v = (g_v - n_v (n_v . g_v)) / |m_v| (0 where m_v = 0), H_t = h_a + h_b + h_c, grad_x = sum over
    (t, corner of x) of (p_next - p_prev) x H_t."""
    p, tri = np.asarray(positions, np.float64), np.asarray(triangles, np.int64)
    h = _h64(sums, cot)
    H = h[:, tri[:, 0]] + h[:, tri[:, 1]] + h[:, tri[:, 2]]
    return _scatter([_cross(p[:, tri[:, (k + 1) % 3]] - p[:, tri[:, (k + 2) % 3]], H) for k in range(3)], tri, p.shape[1])


def forward_rule(positions, triangles):
    """dict(want, bound, zero) per forward output: the float64 value, what its rule allows around it and where the rule asks
    for an exact zero instead; and entries = n_v."""
    p, tri = np.asarray(positions, np.float64), np.asarray(triangles, np.int64)
    V = p.shape[1]
    n_v = incidence(triangles, V)[1]
    a, b, c = (p[:, tri[:, k]] for k in range(3))
    A = _scatter([_abscross(b - a, c - a)] * 3, tri, V)
    eps = (n_v[None, :, None] + 8.0) * E64 * A
    n64, m64 = forward64(positions, triangles)
    M = np.sqrt((m64 * m64).sum(-1, keepdims=True))
    live = M > 0
    an = np.abs(n64)
    nb = U32 * an + (eps + an * (an * eps).sum(-1, keepdims=True)) / np.where(live, M, 1.0) + 4.0 * E64 * an + TINY
    return dict(
        sums=dict(want=m64, bound=U32 * np.abs(m64) + eps + TINY, zero=A == 0),
        normals=dict(want=n64, bound=nb, zero=np.broadcast_to(~live, n64.shape) | (A == 0)),
        entries=n_v,
        A=A,
    )


def backward_rule(positions, triangles, sums, cot):
    """dict(want, bound, zero) of position_grad for the sums and the cotangent the backward kernel is given."""
    p, tri = np.asarray(positions, np.float64), np.asarray(triangles, np.int64)
    V = p.shape[1]
    n_v = incidence(triangles, V)[1]
    m, g = np.abs(np.asarray(sums, np.float64)), np.abs(np.asarray(cot, np.float64))
    s = (m * m).sum(-1, keepdims=True)
    on = s > 0
    sd = np.where(on, s, 1.0)
    habs = np.where(on, (s * g + m * (m * g).sum(-1, keepdims=True)) / (sd * np.sqrt(sd)), 0.0)
    H = habs[:, tri[:, 0]] + habs[:, tri[:, 1]] + habs[:, tri[:, 2]]
    S = _scatter([_abscross(p[:, tri[:, (k + 1) % 3]] - p[:, tri[:, (k + 2) % 3]], H) for k in range(3)], tri, V)
    want = backward_from_sums64(positions, triangles, sums, cot)
    return dict(want=want, bound=U32 * np.abs(want) + (n_v[None, :, None] + 16.0) * E64 * S + TINY, zero=S == 0)


def rule_ratios(got, rule):
    """Per entry, the error over what its rule allows (<= 1 holds it); where the rule asks for an exact zero, 0 for a zero of
    either sign and inf for anything else."""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.abs(got - rule["want"]) / rule["bound"]
    r = np.where(np.isfinite(got), r, np.inf)
    return np.where(rule["zero"], np.where(got == 0, 0.0, np.inf), r)


# ---- the kernels' own order, restated in numpy, with the faults the rules must catch
def _gather(terms, start, n_v, acc, drop_last):
    """[B, V, 3]: a vertex's terms [B, E, 3] added entry after entry, as a lane does, in `acc`."""
    if drop_last:
        n_v = n_v.copy()
        n_v[np.argmax(n_v)] -= 1
    out = np.zeros((terms.shape[0], len(n_v), 3), acc)
    for i in range(int(n_v.max(initial=0))):
        v = np.nonzero(n_v > i)[0]
        out[:, v] += terms[:, start[v] + i].astype(acc)
    return out.astype(np.float64)


def _diff(p32, i, j, diff):
    return (p32[:, i].astype(diff) - p32[:, j].astype(diff)).astype(np.float64)


def kernel_forward_np(positions, triangles, acc=np.float64, diff=np.float64, fused=False, drop_last=False):
    """vertexNormalsKernel restated: (normals, sums) float32, each rounded once.  Faults: acc = float32 accumulators,
    diff = float32 differences, fused = a contracted cross product, drop_last = the longest list loses its last entry."""
    p32, tri = np.asarray(positions, np.float32), np.asarray(triangles, np.int64)
    start, n_v, et, _ = incidence(triangles, p32.shape[1])
    e1, e2 = _diff(p32, tri[:, 1], tri[:, 0], diff), _diff(p32, tri[:, 2], tri[:, 0], diff)
    face = (_cross_fused if fused else _cross)(e1, e2)
    m = _gather(face[:, et], start, n_v, acc, drop_last)
    s = (m * m).sum(-1, keepdims=True)
    on = s > 0
    normals = np.where(on, m * (1.0 / np.sqrt(np.where(on, s, 1.0))), 0.0)
    return normals.astype(np.float32), m.astype(np.float32)


def kernel_backward_np(positions, triangles, sums, cot, acc=np.float64, diff=np.float64, drop_last=False, swap_corner1=False):
    """vertexNormalsBackwardKernel restated: position_grad float32, rounded once; h = (s g - m (m . g)) / (s sqrt s) from the
    float32 sums, H = (h_a + h_b) + h_c.  Faults as above, and swap_corner1 = next and prev exchanged at corner 1."""
    p32, tri = np.asarray(positions, np.float32), np.asarray(triangles, np.int64)
    start, n_v, et, ec = incidence(triangles, p32.shape[1])
    m, g = np.asarray(sums, np.float64), np.asarray(cot, np.float64)
    s = (m * m).sum(-1, keepdims=True)
    on = s > 0
    sd = np.where(on, s, 1.0)
    h = np.where(on, (s * g - m * (m * g).sum(-1, keepdims=True)) * (1.0 / (sd * np.sqrt(sd))), 0.0)
    H = (h[:, tri[:, 0]] + h[:, tri[:, 1]]) + h[:, tri[:, 2]]
    t = tri[et]
    nxt, prv = t[np.arange(len(et)), (ec + 1) % 3], t[np.arange(len(et)), (ec + 2) % 3]
    if swap_corner1:
        nxt, prv = np.where(ec == 1, prv, nxt), np.where(ec == 1, nxt, prv)
    terms = _cross(_diff(p32, nxt, prv, diff), H[:, et])
    return _gather(terms, start, n_v, acc, drop_last).astype(np.float32)


# ---- the entry meshes: name -> (positions [B, V, 3] float32, triangles [T, 3] int32)
def _normal(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def ladder():
    """V = 325 (two workgroups, six groups, the last of five vertices).  Lane l of group 0 has exactly l entries (vertex 0
    none: it is what every padding record names); group 1's longest list is 70 (even); group 3 has no entry at all between
    live groups; group 4's longest list is 1.  Triangles (v, f1, f2), rotated by t mod 3, with the fillers f in the other groups."""
    rng = np.random.default_rng(101)
    V = 325
    owners = np.repeat(np.arange(64), np.arange(64))  # 2016 triangles
    want = np.zeros(V, np.int64)
    want[64:128] = rng.integers(0, 41, size=64)
    want[64 + 17] = 70
    want[256 + rng.choice(64, size=20, replace=False)] = 1
    want[320:325] = [3, 0, 7, 1, 12]
    rest = 2 * len(owners) - want.sum()
    want[128:192] = rng.multinomial(rest, np.full(64, 1.0 / 64))
    slots = np.repeat(np.arange(V), want)
    f = rng.permutation(slots).reshape(-1, 2)
    for t in np.nonzero(f[:, 0] == f[:, 1])[0]:  # (a pair of equal fillers: exchange with the first pair that shares neither)
        o = np.nonzero((f != f[t, 0]).all(axis=1))[0][0]
        f[t, 1], f[o, 1] = f[o, 1], f[t, 1]
    assert (f[:, 0] != f[:, 1]).all()
    tri = np.concatenate([owners[:, None], f], axis=1)[rng.permutation(len(owners))]
    for t in range(len(tri)):
        tri[t] = np.roll(tri[t], t % 3)
    return _normal((2, V, 3), 102), tri.astype(np.int32)


def soup(V, T, seed, B=2):
    """T random triangles of distinct vertices chosen with weight (1 + i)^-0.8 (valences from 0 to a fifth of 3 T); N(0, 1)."""
    rng = np.random.default_rng(seed)
    w = (1.0 + np.arange(V)) ** -0.8
    tri = np.stack([rng.choice(V, size=3, replace=False, p=w / w.sum()) for _ in range(T)]).astype(np.int32)
    return _normal((B, V, 3), seed + 1), tri


def books():
    """70 disjoint pairs of faces of size 1 .. 3 folded almost shut around a shared edge, fold angles 10^-2 .. 10^-5: at the
    two vertices of the edge the face vectors nearly cancel (A / |m| from 10^2 to beyond 10^5 -- what CAP keeps out of MESHES)."""
    rng = np.random.default_rng(111)
    pos, tri = [], []
    for k, theta in enumerate(np.logspace(-2, -5, 70)):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        L, c = rng.uniform(1.0, 3.0, size=2), rng.normal(size=3)
        local = np.array([[-0.5 * L[0], 0, 0], [0.5 * L[0], 0, 0], [0.1, L[1], 0], [0.1, L[1] * np.cos(theta), L[1] * np.sin(theta)]])
        pos.append(local @ q.T + c)
        tri += [[4 * k, 4 * k + 1, 4 * k + 2], [4 * k + 1, 4 * k, 4 * k + 3]]
    pos = np.concatenate(pos)
    return np.stack([pos, pos * 1.7 + 0.3]).astype(np.float32), np.asarray(tri, np.int32)


def cm():
    """Centimetres, away from the origin: the 21 x 12 torus and soup_300 side by side, times 100 and moved by (0, 150, 20)."""
    tp, tt = torus(21, 12, 2, 121)
    sp, stri = soup(300, 900, 300)
    pos = np.concatenate([tp.astype(np.float64), sp.astype(np.float64)], axis=1) * 100.0 + np.array([0.0, 150.0, 20.0])
    return pos.astype(np.float32), np.concatenate([tt, stri + tp.shape[1]]).astype(np.int32)


def _is_degenerate(tri):
    return (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])


def mixed():
    """soup_70 (vertices 0 .. 69) with triangles (a, a, b), (a, b, a), (b, a, a), (a, a, a) put first, in the middle and last in
    the triangle list (so first, in the middle and last in the lists of a and b); vertices 70 .. 75 sit on such triangles only;
    vertices 76 .. 99 carry twelve triangles each followed at once by its reversed copy (a, c, b); vertices 100 .. 104 are isolated."""
    pos, tri = soup(70, 200, 70)
    rng = np.random.default_rng(131)

    def degenerate(k):
        a, b = rng.choice(70, size=2, replace=False)
        out = [[a, a, b], [a, b, a], [b, a, a], [a, a, a], [70 + k, 70 + k, a], [b, 71 + k, 71 + k], [0, 3, 0], [3, 0, 0]]
        return np.asarray(out)

    pairs = []
    for i in range(12):
        a, b, c = 76 + 2 * i, 76 + 2 * i + 1, 76 + (2 * i + 2) % 24
        pairs += [[a, b, c], [a, c, b]]
    tri = np.concatenate([degenerate(0), tri[:100], degenerate(2), tri[100:150], np.asarray(pairs), tri[150:], degenerate(4)]).astype(np.int32)
    return np.concatenate([pos, _normal((2, 35, 3), 132)], axis=1), tri


def v1():
    return np.array([[[0.25, -1.5, 3.0]], [[1.0, 2.0, -0.5]]], np.float32), np.zeros((1, 3), np.int32)


ENTRY_MESHES = {"ladder": ladder, "soup_70": lambda: soup(70, 200, 70), "soup_300": lambda: soup(300, 900, 300), "books": books, "cm": cm, "mixed": mixed, "v1": v1}


def arbitrary_sums(shape, seed):
    """(sums, cotangent) [B, V, 3] float32 no forward gives: sums of magnitude 10^U(-12, 12), every seventh one zero; cotangents
    N(0, 1), every third one its sum times a power of two (exactly parallel, of magnitude about 1)."""
    rng = np.random.default_rng(seed)
    B, V = shape[:2]
    sums = (rng.normal(size=shape) * 10.0 ** rng.uniform(-12.0, 12.0, size=(B, V, 1))).astype(np.float32)
    flat = np.arange(B * V).reshape(B, V)
    sums[flat % 7 == 0] = 0.0
    cot = rng.normal(size=shape).astype(np.float32)
    par = (flat % 3 == 1) & (flat % 7 != 0)
    k = -np.floor(np.log2(np.abs(sums[par]).max(axis=-1, keepdims=True))).astype(np.int32)
    cot[par] = np.ldexp(sums[par], k)
    return sums, cot


def entry_case(name):
    """(positions, triangles, cotangent) of an entry mesh."""
    pos, tri = ENTRY_MESHES[name]()
    return pos, tri, cotangent(pos.shape, 7)
