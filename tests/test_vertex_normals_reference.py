"""The vertex-normal reference (tests/vertex_normals_reference.py) on its own, on the CPU: hand cases with normals known in
closed form, its float64 gradient against central differences and against the formulas of include/mmx.h written as loops, and
the condition of admission of the parity meshes -- on every one the float32 reference is within 1e-6 of the float64 one."""
import numpy as np
import pytest
import torch

from tests import vertex_normals_reference as ref


def _normals64(pos, tri):
    return ref.vertex_normals(torch.as_tensor(np.asarray(pos, np.float64))[None], torch.as_tensor(np.asarray(tri, np.int64)))[0].numpy()


def test_single_triangle():
    p = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    assert np.allclose(_normals64(p, [[0, 1, 2]]), [[0, 0, 1]] * 3, atol=1e-15)
    assert np.allclose(_normals64(p, [[0, 2, 1]]), [[0, 0, -1]] * 3, atol=1e-15)  # the corner order decides the side
    q = np.array([[0.1, 0.2, -0.3], [0.9, 0.1, 0.2], [0.3, 0.8, 0.4]])
    c = np.cross(q[1] - q[0], q[2] - q[0])
    n, m = ref.vertex_normals(torch.as_tensor(q)[None], torch.tensor([[0, 1, 2]]), want_sums=True)
    assert np.allclose(m[0].numpy(), [c] * 3, rtol=1e-15) and np.allclose(n[0].numpy(), [c / np.linalg.norm(c)] * 3, rtol=1e-15)


def test_flat_quad_and_an_isolated_vertex():
    p = np.array([[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [1.0, 2.0, 0.5], [0.0, 2.0, 0.5], [7.0, 7.0, 7.0]])
    n = _normals64(p, [[0, 1, 2], [0, 2, 3]])
    assert np.allclose(n[:4], [[0, 0, 1]] * 4, atol=1e-15)
    assert np.array_equal(n[4], [0, 0, 0])  # no triangle: zeros, not NaN
    assert np.array_equal(_normals64(p, [[0, 0, 1]]), np.zeros((5, 3)))  # a degenerate triangle only: zeros everywhere


def test_regular_tetrahedron():
    """Four equal faces turned outwards: a vertex's normal is the sum of its three faces', by symmetry its own direction."""
    p = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    tri = []
    for skip in range(4):
        a, b, c = [v for v in range(4) if v != skip]
        if np.cross(p[b] - p[a], p[c] - p[a]) @ (p[a] + p[b] + p[c]) < 0:
            b, c = c, b
        tri.append([a, b, c])
    assert np.allclose(_normals64(p, tri), p / np.sqrt(3.0), atol=1e-15)
    # area weighting: stretch one face's far vertex and the shared vertices lean towards the larger faces
    q = p.copy()
    q[0] *= 3.0
    n = _normals64(q, tri)
    faces = np.array([np.cross(q[b] - q[a], q[c] - q[a]) for a, b, c in tri])
    want = np.array([faces[[v in t for t in tri]].sum(0) for v in range(4)])
    assert np.allclose(n, want / np.linalg.norm(want, axis=1, keepdims=True), atol=1e-15)


def test_float64_gradient_against_central_differences_and_the_header_formulas():
    pos, tri = ref.MESHES["torus_8x4_b1"]()
    pos = pos[0].astype(np.float64)
    cot = ref.cotangent(pos.shape, 3).astype(np.float64)
    got = ref.vjp_autograd(pos[None], tri, cot[None], torch.float64)
    loss = lambda p: float((_normals64(p, tri) * cot).sum())
    fd, eps = np.zeros_like(pos), 1e-6
    for i in range(pos.size):
        d = np.zeros(pos.size)
        d[i] = eps
        fd.flat[i] = (loss(pos + d.reshape(pos.shape)) - loss(pos - d.reshape(pos.shape))) / (2 * eps)
    scale = np.abs(got["position_grad"]).max()
    assert np.abs(got["position_grad"][0] - fd).max() <= 1e-7 * scale  # (truncation eps^2 x third derivative, rounding 1e-16 / eps)
    n, m, grad = ref.vjp_np(pos, tri, cot)
    assert np.abs(n - got["normals"][0]).max() <= 1e-14 and np.abs(m - got["sums"][0]).max() <= 1e-14 * np.abs(m).max()
    assert np.abs(grad - got["position_grad"][0]).max() <= 1e-13 * scale


def test_vjp_np_with_isolated_and_repeated_corners():
    p = np.random.default_rng(1).normal(size=(6, 3))
    tri = np.array([[0, 1, 2], [2, 1, 3], [4, 4, 0], [3, 0, 2]])  # vertex 5 isolated, vertex 4 on a degenerate triangle only
    cot = np.random.default_rng(2).normal(size=(6, 3))
    got = ref.vjp_autograd(p[None], tri, cot[None], torch.float64)
    n, m, grad = ref.vjp_np(p, tri, cot)
    assert np.allclose(n, got["normals"][0], atol=1e-14) and np.allclose(grad, got["position_grad"][0], atol=1e-13)
    assert not n[4:].any() and not grad[5].any()


@pytest.mark.parametrize("name", list(ref.MESHES))
def test_float32_reference_holds_the_cap_on_every_parity_mesh(name):
    pos, tri, cot = ref.parity_case(name)
    w64, w32 = ref.vjp_autograd(pos, tri, cot, torch.float64), ref.vjp_autograd(pos, tri, cot, torch.float32)
    for key in ("normals", "sums", "position_grad"):
        d = ref.dist(w32[key], w64[key]).max()
        print(f"{name}/{key}: d32 {d:.3e}")
        assert 0 < d <= ref.CAP, (name, key, d)


def test_rings():
    pos, tri = ref.MESHES["edge_v63"]()  # a 10 x 6 grid: wide enough for a 2-ring not to meet itself around the torus
    one, two = ref.rings(tri, pos.shape[1], 15)
    assert one.sum() == 7 and one[15]  # valence 6
    assert two.sum() == 19 and (two | one).sum() == 19 and not two[60:].any()
