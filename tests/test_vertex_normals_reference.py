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


# ---- the per-entry rules of tests/test_gpu_vertex_normals_entries.py: the meshes, soundness, teeth, the backward reference
def _variants(name):
    """(label, positions, triangles, sums given to the backward or None = the forward's, cotangent): what the GPU file runs."""
    pos, tri, cot = ref.entry_case(name)
    out = [("forward_sums", pos, tri, None, cot)]
    if name in ("ladder", "soup_70"):
        sums, g = ref.arbitrary_sums(pos.shape, 9)
        out.append(("arbitrary_sums", pos, tri, sums, g))
    return out


def _restated_worst(pos, tri, sums, cot, **fault):
    """Worst error / bound per output of the numpy restatement of the kernels (with the planted fault)."""
    fwd = {k: v for k, v in fault.items() if k in ("acc", "diff", "fused", "drop_last")}
    bwd = {k: v for k, v in fault.items() if k in ("acc", "diff", "drop_last", "swap_corner1")}
    normals, m = ref.kernel_forward_np(pos, tri, **fwd)
    given = m if sums is None else sums
    got = dict(normals=normals, sums=m, position_grad=ref.kernel_backward_np(pos, tri, given, cot, **bwd))
    rules = ref.forward_rule(pos, tri)
    rules["position_grad"] = ref.backward_rule(pos, tri, given, cot)
    return {key: float(ref.rule_ratios(got[key], rules[key]).max()) for key in ref.KEYS}


def test_ladder_has_every_list_length_and_an_empty_group():
    pos, tri = ref.ladder()
    assert pos.shape == (2, 325, 3)
    t = ref.capi.host_mesh_tables(325, tri)
    n = np.diff(t["vertex_start"])
    assert np.array_equal(n[:64], np.arange(64)) and n[0] == 0  # lane l of group 0: l entries; vertex 0 few (none)
    assert n[64:128].max() >= 64 and n[64:128].max() % 2 == 0 and n[:64].max() % 2 == 1
    assert n[192:256].sum() == 0 and n[128:192].max() > 0 and n[256:320].max() == 1  # an empty group between live ones; longest list 1
    assert n[320:].max() > 1 and (n[320:] == 0).any() and t["max_valence"] == n.max()
    assert set(t["entry_corner"][t["vertex_start"][63] : t["vertex_start"][64]]) == {0, 1, 2}


def test_the_other_entry_meshes_are_what_they_say():
    for name, V, T in (("soup_70", 70, 200), ("soup_300", 300, 900)):
        pos, tri = ref.ENTRY_MESHES[name]()
        n = ref.incidence(tri, V)[1]
        assert pos.shape[1:] == (V, 3) and tri.shape == (T, 3) and n.min() == 0 and n.max() > (60 if V == 70 else 180) and n[0] == n.max()
        assert not ref._is_degenerate(tri).any()
    pos, tri = ref.books()
    rule = ref.forward_rule(pos, tri)
    cond = np.linalg.norm(rule["A"], axis=-1) / np.linalg.norm(rule["sums"]["want"], axis=-1)
    assert tri.shape == (140, 3) and cond.max() > 1e4 and (cond > 1e3).sum() >= 40 and cond.min() < 3.0
    w64, w32 = ref.vjp_autograd(pos, tri, ref.cotangent(pos.shape, 7), torch.float64), ref.vjp_autograd(pos, tri, ref.cotangent(pos.shape, 7), torch.float32)
    assert ref.dist(w32["normals"], w64["normals"]).max() > 100 * ref.CAP  # what CAP keeps out of MESHES
    pos, tri = ref.cm()
    assert pos.shape == (2, 552, 3) and 100 < np.abs(pos[..., 1]).mean() < 200 and np.abs(pos).max() > 250
    pos, tri = ref.mixed()
    start, n, et, ec = ref.incidence(tri, pos.shape[1])
    dead = ref._is_degenerate(tri)
    assert dead.sum() == 24 and (n[100:] == 0).all() and (n[70:76] > 0).all() and dead[et[start[70] : start[76]]].all()
    for v in (0, 3):  # degenerate entries first, in the middle and last in a live vertex's list
        d = dead[et[start[v] : start[v + 1]]]
        assert d[0] and d[-1] and d[1:-1].any() and not d.all()
    m = ref.kernel_forward_np(pos, tri)[1]
    assert not m[:, 70:].any() and rule["A"].min() >= 0 and ref.forward_rule(pos, tri)["A"][:, 76:100].min() > 0  # exact cancellation, not absence
    pos, tri = ref.v1()
    assert pos.shape[1:] == (1, 3) and tri.tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("name", list(ref.ENTRY_MESHES))
def test_the_restated_kernels_hold_every_rule(name):
    """Soundness: float64 in the kernels' own order, rounded once, is inside every bound -- mostly by the u |x64| of that rounding."""
    for label, pos, tri, sums, cot in _variants(name):
        worst = _restated_worst(pos, tri, sums, cot)
        print(f"{name}/{label}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, (name, label, worst)


def test_planted_faults_break_the_rules():
    """Teeth.  By a factor of at least 10: float32 accumulators (every random mesh, the folds, the arbitrary sums), float32
    differences on cm.  By exact zeros or errors of order 1: a fused cross product on mixed, the last entry of the longest list
    dropped on ladder, next and prev exchanged at corner 1."""
    worst = {}
    for name in ("ladder", "soup_70", "soup_300", "books", "cm"):
        for label, pos, tri, sums, cot in _variants(name):
            w = worst[f"float32_accumulators/{name}/{label}"] = _restated_worst(pos, tri, sums, cot, acc=np.float32)
            assert w["position_grad"] >= 10.0 and (sums is not None or min(w.values()) >= 10.0), (name, label, w)
    pos, tri, cot = ref.entry_case("cm")
    w = worst["float32_differences/cm"] = _restated_worst(pos, tri, None, cot, diff=np.float32)
    assert min(w.values()) >= 10.0, w
    pos, tri, cot = ref.entry_case("mixed")
    w = worst["fused_cross/mixed"] = _restated_worst(pos, tri, None, cot, fused=True)
    assert w["normals"] == np.inf, w  # a nonzero where a zero is asked
    fused = ref.kernel_forward_np(pos, tri, fused=True)[1]
    assert fused[:, 70:].any() and not ref.kernel_forward_np(pos, tri)[1][:, 70:].any()  # (where a product of two differences is not exact)
    for label, pos, tri, sums, cot in _variants("ladder"):
        w = worst[f"last_entry_dropped/ladder/{label}"] = _restated_worst(pos, tri, sums, cot, drop_last=True)
        assert w["position_grad"] >= 1e5 if sums is None else w["position_grad"] <= 1.0, w  # (next to sums of 10^-12 the dropped term is below the float32 rounding of the result)
        assert w["sums"] >= 1e5 and w["normals"] >= 1e5, w
    for name in ("ladder", "soup_70", "books"):
        for label, pos, tri, sums, cot in _variants(name):
            w = worst[f"next_prev_exchanged_at_corner_1/{name}/{label}"] = _restated_worst(pos, tri, sums, cot, swap_corner1=True)
            assert w["position_grad"] >= 1e6 and max(w["sums"], w["normals"]) <= 1.0, (name, label, w)
    for k, w in worst.items():
        print(f"{k}: " + "  ".join(f"{key} {v:.3g}" for key, v in w.items()))


@pytest.mark.parametrize("name", list(ref.ENTRY_MESHES))
def test_backward_from_given_sums_is_autograd_when_the_sums_are_the_forwards(name):
    pos, tri, cot = ref.entry_case(name)
    w = ref.vjp_autograd(pos, tri, cot, torch.float64)
    got = ref.backward_from_sums64(pos, tri, w["sums"], cot)  # unrounded float64 sums
    scale = np.abs(w["position_grad"]).max(axis=(1, 2), keepdims=True)
    assert np.all(np.abs(got - w["position_grad"]) <= 1e-12 * scale), name
    if name != "mixed":  # (torch's cross product leaves a rounding error where a triangle meets its reversed copy)
        assert np.abs(ref.forward64(pos, tri)[1] - w["sums"]).max() <= 1e-14 * np.abs(w["sums"]).max()


def test_arbitrary_sums_are_what_they_say():
    sums, cot = ref.arbitrary_sums((2, 325, 3), 9)
    mag = np.abs(sums.astype(np.float64)).max(-1)
    assert (mag == 0).sum() == len(range(0, 650, 7)) and mag[mag > 0].min() < 1e-10 and mag.max() > 1e10
    par = np.linalg.norm(np.cross(sums.astype(np.float64), cot.astype(np.float64)), axis=-1) == 0
    assert (par & (mag > 0)).sum() >= 650 // 4 and 0.5 <= np.abs(cot[par & (mag > 0)]).max(-1).min() and np.abs(cot[par & (mag > 0)]).max() < 2.0
