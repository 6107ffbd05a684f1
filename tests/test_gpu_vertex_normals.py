"""Vertex normals on the GPU (mmx_vertex_normals / mmx_vertex_normals_backward; capi.Mesh, autograd.vertex_normals,
geometry.compute_vertex_normals) against the float64 torch reference of tests/vertex_normals_reference.py.

Bound.  The distance is max|x - x64| / max|x64| per instance.  The float32 reference (the same torch code in float32, on the
CPU) has a distance d32 of its own from the float64 one; the GPU's normals, sums and position gradient must stay within
4 x the largest d32 over the test's instances (the factor covers the different summation order: torch scatters triangle by
triangle, the kernels gather vertex by vertex).  Every parity mesh holds d32 <= 1e-6 (tests/test_vertex_normals_reference.py).
Positions are float32 and go to the GPU and to both references alike; cotangents are standard-normal; fixed seeds.

Measured on an MI355X (largest distance over the instances, gpu | d32 | bound = 4 x d32; profiles/vertex_normals_parity.json,
written through MMX_PARITY_OUT):
    single_triangle        normals 4.88e-08 | 1.33e-07 | 5.32e-07   sums 3.47e-08 | 1.03e-07 | 4.13e-07   position_grad 6.78e-08 | 1.59e-07 | 6.36e-07
    torus_8x4_b1           normals 2.94e-08 | 1.24e-07 | 4.95e-07   sums 4.34e-08 | 9.06e-08 | 3.62e-07   position_grad 6.77e-08 | 2.49e-07 | 9.98e-07
    torus_8x4_b5           normals 2.98e-08 | 1.24e-07 | 4.95e-07   sums 4.47e-08 | 1.06e-07 | 4.26e-07   position_grad 6.77e-08 | 2.49e-07 | 9.98e-07
    fan_1000               normals 2.98e-08 | 1.44e-07 | 5.75e-07   sums 5.29e-09 | 5.83e-07 | 2.33e-06   position_grad 5.13e-08 | 5.62e-07 | 2.25e-06
    torus_64x32_offset     normals 2.98e-08 | 1.32e-07 | 5.28e-07   sums 4.66e-08 | 1.09e-07 | 4.38e-07   position_grad 4.49e-08 | 1.22e-07 | 4.89e-07
    edge_v63               normals 2.92e-08 | 1.03e-07 | 4.11e-07   sums 3.17e-08 | 8.41e-08 | 3.37e-07   position_grad 4.82e-08 | 2.78e-07 | 1.11e-06
    edge_v64               normals 2.96e-08 | 1.14e-07 | 4.56e-07   sums 3.19e-08 | 8.29e-08 | 3.32e-07   position_grad 4.63e-08 | 1.88e-07 | 7.51e-07
    edge_v65               normals 2.97e-08 | 8.45e-08 | 3.38e-07   sums 2.94e-08 | 9.74e-08 | 3.90e-07   position_grad 3.71e-08 | 1.87e-07 | 7.49e-07
    edge_v255              normals 2.98e-08 | 1.25e-07 | 4.98e-07   sums 5.18e-08 | 1.01e-07 | 4.05e-07   position_grad 6.69e-08 | 1.66e-07 | 6.63e-07
    edge_v256              normals 2.98e-08 | 1.13e-07 | 4.52e-07   sums 5.09e-08 | 8.78e-08 | 3.51e-07   position_grad 3.68e-08 | 1.45e-07 | 5.80e-07
    edge_v257              normals 2.98e-08 | 1.23e-07 | 4.92e-07   sums 4.86e-08 | 1.11e-07 | 4.43e-07   position_grad 4.46e-08 | 1.69e-07 | 6.78e-07
    end_to_end_chain24     normals 1.18e-05 | 9.37e-06 | 3.75e-05   theta_grad 1.27e-05 | 3.39e-05 | 1.36e-04
Every figure is inside its bound.  The kernels take differences, cross products and sums in double and round each output once:
they sit at the rounding of the result where the float32 reference carries the rounding of every step.  The end-to-end mesh is
folded over itself by the poses (rotations of +-1 rad on a 24-joint chain), which is what lifts both chains to 1e-5 there.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import autograd as mauto
from momentum_amd import capi, geometry, make_test_character, make_test_mesh, make_test_skinned_mesh
from tests import skeleton_state_reference as fk
from tests import skinning_reference as skin_ref
from tests import vertex_normals_reference as ref

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT = 1
_parity = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    """MMX_PARITY_OUT=<file>: the measured distances of this run as JSON (how profiles/vertex_normals_parity.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _parity:
        with open(out, "w") as f:
            json.dump(dict(unit="max|x - x_ref64| / max|x_ref64| per instance, largest over the instances; bound = 4 x d32", shapes=_parity), f, indent=1)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _run_gpu(mesh, pos, cot):
    p, g = _cuda(pos), _cuda(cot)
    normals, sums = mesh.vertex_normals(p, want_sums=True)
    grad = mesh.vertex_normals_backward(p, sums, g)
    return dict(normals=normals.cpu().numpy(), sums=sums.cpu().numpy(), position_grad=grad.cpu().numpy())


def _compare(name, got, want64, want32, finite=True):
    for key in got:
        d32, dg = ref.dist(want32[key], want64[key]), ref.dist(got[key], want64[key])
        _parity[f"{name}/{key}"] = dict(gpu=float(dg.max()), d32=float(d32.max()), bound=float(4 * d32.max()))
        print(f"{name}/{key}: gpu {dg.max():.3e}  d32 {d32.max():.3e}  bound {4 * d32.max():.3e}")
    for key in got:
        assert not finite or np.isfinite(got[key]).all(), (name, key)
        p = _parity[f"{name}/{key}"]
        assert p["gpu"] <= p["bound"], (name, key, p)


@pytest.mark.parametrize("name", list(ref.MESHES))
def test_forward_and_backward_match_the_reference(torch_cuda, name):
    pos, tri, cot = ref.parity_case(name)
    B, V = pos.shape[:2]
    mesh = capi.Mesh(tri, V)
    got = _run_gpu(mesh, pos, cot)
    _compare(name, got, ref.vjp_autograd(pos, tri, cot, torch.float64), ref.vjp_autograd(pos, tri, cot, torch.float32))
    used = np.zeros(V, bool)
    used[tri.reshape(-1)] = True
    for key in got:  # a vertex of no triangle: exact (positive) zeros everywhere
        assert np.all(got[key][:, ~used] == 0.0) and not np.signbit(got[key][:, ~used]).any(), key
    assert np.abs(np.linalg.norm(got["normals"][:, used].astype(np.float64), axis=-1) - 1.0).max() <= 2.0**-22
    if name.startswith("edge_v"):
        assert (~used).sum() == V - (60 if V < 100 else 252)
    # the forward without sums writes the same normals
    assert np.array_equal(mesh.vertex_normals(_cuda(pos)).cpu().numpy(), got["normals"])


def test_degenerate_triangles_only_give_exact_zeros(torch_cuda):
    V, B = 70, 2
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, V, size=40), rng.integers(0, V, size=40)
    tri = np.stack([a, a, b], axis=1).astype(np.int32)
    tri[::3] = tri[::3][:, [2, 0, 1]]  # (b, a, a) and, below, (a, b, a) as well
    tri[1::3] = tri[1::3][:, [0, 2, 1]]
    pos = rng.normal(size=(B, V, 3)).astype(np.float32)
    got = _run_gpu(capi.Mesh(tri, V), pos, ref.cotangent(pos.shape, 6))
    for key in got:
        assert np.array_equal(got[key].view(np.uint32), np.zeros_like(got[key]).view(np.uint32)), key


def test_nan_position_stays_in_its_rings(torch_cuda):
    pos, tri = ref.torus(21, 12, 3, 61, isolated=4)
    B, V = pos.shape[:2]
    cot = ref.cotangent(pos.shape, 62)
    mesh = capi.Mesh(tri, V)
    clean = _run_gpu(mesh, pos, cot)
    bad_b, bad_v = 1, 100
    one, two = ref.rings(tri, V, bad_v)
    assert one.sum() == 7 and two.sum() == 19
    for value in (np.nan, np.inf):
        bad = pos.copy()
        bad[bad_b, bad_v, 1] = value
        got = _run_gpu(mesh, bad, cot)
        for key, ring in (("normals", one), ("sums", one), ("position_grad", two)):
            if key == "sums":  # (a face vector's component that does not read the bad coordinate stays finite: the sums are raw)
                assert (~np.isfinite(got[key][bad_b, ring])).any(axis=-1).all(), (key, value)
            else:
                assert np.isnan(got[key][bad_b, ring]).all(), (key, value)  # exactly on the ring, every component ...
            rest = np.ascontiguousarray(got[key][bad_b, ~ring]), np.ascontiguousarray(clean[key][bad_b, ~ring])
            assert np.array_equal(rest[0].view(np.uint32), rest[1].view(np.uint32)), (key, value)  # ... and nowhere else
            for b in (0, 2):
                assert np.array_equal(got[key][b].view(np.uint32), clean[key][b].view(np.uint32)), (key, value, b)
    # a NaN cotangent: the gradient is NaN on that vertex's closed 1-ring only (H_t of its triangles)
    g = cot.copy()
    g[2, bad_v, 0] = np.nan
    got = _run_gpu(mesh, pos, g)
    assert np.isnan(got["position_grad"][2, one]).all()
    assert np.array_equal(got["position_grad"][2, ~one], clean["position_grad"][2, ~one])
    assert np.array_equal(got["position_grad"][:2], clean["position_grad"][:2])


def test_a_row_depends_on_its_instance_only_and_out_buffers_are_honoured(torch_cuda):
    pos, tri = ref.MESHES["edge_v257"]()
    V = pos.shape[1]
    pos5 = ref.instances(pos[0], 5, 71, 0.01)
    cot5 = ref.cotangent(pos5.shape, 72)
    mesh = capi.Mesh(tri, V)
    alone = _run_gpu(mesh, pos5[3:4], cot5[3:4])
    five = _run_gpu(mesh, pos5, cot5)
    again = _run_gpu(mesh, pos5, cot5)
    for key in five:
        assert np.array_equal(five[key][3].view(np.uint32), alone[key][0].view(np.uint32)), key  # row 0 of B = 1 is row 3 of B = 5
        assert np.array_equal(five[key].view(np.uint32), again[key].view(np.uint32)), key  # two runs
    # out= buffers
    p, g = _cuda(pos5), _cuda(cot5)
    out = torch.full((5, V, 3), -7.25, device="cuda")
    r = mesh.vertex_normals(p, out=out)
    assert r is out and np.array_equal(out.cpu().numpy(), five["normals"])
    n2, sums = mesh.vertex_normals(p, want_sums=True, out=out)
    assert n2 is out
    gout = torch.full((5, V, 3), -7.25, device="cuda")
    assert mesh.vertex_normals_backward(p, sums, g, out=gout) is gout and np.array_equal(gout.cpu().numpy(), five["position_grad"])
    assert mesh.V == V and mesh.T == len(tri) and capi.lib().mmx_mesh_num_vertices(mesh._h) == V and capi.lib().mmx_mesh_num_triangles(mesh._h) == len(tri)


def test_autograd_function_and_compute_vertex_normals(torch_cuda):
    pos, tri = ref.MESHES["torus_8x4_b5"]()
    B, V = pos.shape[:2]
    cot = ref.cotangent(pos.shape, 81)
    mesh = capi.Mesh(tri, V)
    want = _run_gpu(mesh, pos, cot)
    p = _cuda(pos).requires_grad_(True)
    n = mauto.vertex_normals(mesh, p)
    assert n.grad_fn is not None
    (grad,) = torch.autograd.grad((n * _cuda(cot)).sum(), p)
    assert np.array_equal(n.detach().cpu().numpy(), want["normals"]) and np.array_equal(grad.cpu().numpy(), want["position_grad"])
    # without requires_grad, or under no_grad: the plain forward, no graph node
    assert mauto.vertex_normals(mesh, _cuda(pos)).grad_fn is None
    with torch.no_grad():
        assert mauto.vertex_normals(mesh, p).grad_fn is None
    # the reference's call shape: a handle (the loop form) or the triangles themselves, batched or a single element
    for triangles in (mesh, torch.from_numpy(tri).cuda(), tri, torch.from_numpy(tri.astype(np.int64))):
        assert np.array_equal(geometry.compute_vertex_normals(_cuda(pos), triangles).cpu().numpy(), want["normals"])
    single = geometry.compute_vertex_normals(_cuda(pos[2]), tri)
    assert single.shape == (V, 3) and np.array_equal(single.cpu().numpy(), want["normals"][2])
    q = _cuda(pos).requires_grad_(True)
    (geometry.compute_vertex_normals(q, tri) * _cuda(cot)).sum().backward()
    assert np.array_equal(q.grad.cpu().numpy(), want["position_grad"])


def test_end_to_end_from_theta(torch_cuda):
    """theta -> state -> vertices -> normals and back, one kernel per stage in each direction, against the float64 chain of the
    three reference modules; the bound is 4 x the float32 chain's distance."""
    rig = make_test_character(24)
    skin, tri = make_test_skinned_mesh(rig, 32, 16, 4, 91)
    V, B = skin.rest.shape[0], 3
    assert V == 512
    rh = capi.RigHandle(rig, 0)
    sk = capi.Skin(rh, skin.joint, skin.weight, skin.inverse_bind, skin.rest)
    mesh = capi.Mesh(tri, V)
    pb = capi.Problem(rh, B, [0], [])
    theta, _ = fk.random_inputs(rig, B, seed=92)
    cot = ref.cotangent((B, V, 3), 93)
    th = _cuda(theta).requires_grad_(True)
    normals = mauto.vertex_normals(mesh, mauto.skin_points(sk, mauto.skeleton_state(pb, th)))
    (normals * _cuda(cot)).sum().backward()

    def chain(dtype):
        rt = fk.RigTensors(rig, dtype)
        st = skin_ref.SkinTensors(skin.joint, skin.weight, skin.inverse_bind, skin.rest, rig.num_joints, dtype)
        x = torch.as_tensor(theta, dtype=dtype).clone().requires_grad_(True)
        n = ref.vertex_normals(skin_ref.skin_points(st, fk.skeleton_state(rt, x)), torch.as_tensor(tri.astype(np.int64)))
        (n * torch.as_tensor(cot, dtype=dtype)).sum().backward()
        return dict(normals=n.detach().numpy(), theta_grad=x.grad.numpy())

    _compare("end_to_end_chain24", dict(normals=normals.detach().cpu().numpy(), theta_grad=th.grad.cpu().numpy()), chain(torch.float64), chain(torch.float32))


def test_normals_feed_find_closest_points(torch_cuda):
    """A torus against itself shifted by a tenth of an edge, with the normals of both from the kernel: every valid index is the
    brute-force answer computed in torch from the same normals."""
    m = make_test_mesh(24, 12, 0.1, 95)
    V = m.positions.shape[0]
    clean = make_test_mesh(24, 12, 0.0, 95).positions
    edge = float(np.linalg.norm(clean[1] - clean[0]))
    src = _cuda(m.positions[None])
    tgt = _cuda((m.positions + np.array([0.1 * edge, 0.0, 0.0], np.float32))[None])
    mesh = capi.Mesh(m.triangles, V)
    ns, nt = geometry.compute_vertex_normals(src, mesh), geometry.compute_vertex_normals(tgt, mesh)
    min_dot = 0.5
    points, index, valid = geometry.find_closest_points(src, ns, tgt, nt, max_dist=3.0 * edge, min_normal_dot=min_dot)
    # brute force with the kernel's arithmetic (include/mmx.h): float32 differences first, then fma chains -- an fma is taken in
    # float64, where the product of two float32 is exact, and rounded once -- ordered comparisons, the lowest index among equals
    fma32 = lambda x, y, z: (x.double() * y.double() + z.double()).float()
    chain = lambda ax, ay, az, bx, by, bz: fma32(az, bz, fma32(ay, by, ax * bx))
    d = src[0][:, None, :] - tgt[0][None, :, :]
    d2 = chain(d[..., 0], d[..., 1], d[..., 2], d[..., 0], d[..., 1], d[..., 2])
    col = lambda t, c: t[0][:, None, c].expand(V, V)
    row = lambda t, c: t[0][None, :, c].expand(V, V)
    dots = chain(col(ns, 0), col(ns, 1), col(ns, 2), row(nt, 0), row(nt, 1), row(nt, 2))
    maxd2 = torch.tensor(3.0 * edge, dtype=torch.float32, device="cuda").square()
    masked = torch.where((dots >= min_dot) & (d2 <= maxd2), d2, torch.full_like(d2, float("inf")))
    best = masked.min(dim=1).values
    want_valid = torch.isfinite(best)
    first = (masked == best[:, None]).float().argmax(dim=1)  # (the first of the equal minima)
    assert torch.equal(valid[0], want_valid) and valid[0].sum().item() >= V - 4
    got = index[0].long()
    assert torch.equal(got[want_valid], first[want_valid])
    assert torch.all(index[0][~want_valid] == -1).item()
    assert torch.equal(points[0][want_valid], tgt[0][got[want_valid]])
    # most sources find the vertex they were shifted from, and a front never matches a back: the winner's dot is >= min_dot
    every = torch.arange(V, device="cuda")[want_valid]
    assert (got[want_valid] == every).float().mean().item() > 0.9
    assert bool((dots[every, got[want_valid]] >= min_dot).all())
    # without the normal test the inner side of the tube may win: the normals decide something on this mesh
    assert bool((dots < min_dot).any())


def test_graph_capture_from_the_first_call(torch_cuda):
    pos, tri = ref.MESHES["edge_v257"]()
    B, V = pos.shape[:2]
    cot = ref.cotangent(pos.shape, 97)
    mesh = capi.Mesh(tri, V)  # no call on this handle before the capture
    p, g = _cuda(pos), _cuda(cot)
    normals, sums, grad = (torch.empty_like(p) for _ in range(3))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L = capi.lib()
        capi._check(L.mmx_vertex_normals(mesh._h, B, capi._dev(p), capi._dev(normals), capi._dev(sums), capi._stream_ptr()))
        capi._check(L.mmx_vertex_normals_backward(mesh._h, B, capi._dev(p), capi._dev(sums), capi._dev(g), capi._dev(grad), capi._stream_ptr()))
    for seed in (98, 99):  # replayed on new positions
        new = ref.instances(pos[0], B, seed, 0.01)
        p.copy_(_cuda(new))
        graph.replay()
        torch.cuda.synchronize()
        eager = _run_gpu(mesh, new, cot)
        for key, t in (("normals", normals), ("sums", sums), ("position_grad", grad)):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), eager[key].view(np.uint32)), (key, seed)


def test_refusals_touch_no_output(torch_cuda):
    pos, tri = ref.MESHES["torus_8x4_b5"]()
    B, V = pos.shape[:2]
    mesh = capi.Mesh(tri, V)
    p = _cuda(pos)
    a, b, c = (torch.full((B, V, 3), -7.25, device="cuda") for _ in range(3))
    L, null, d = capi.lib(), C.c_void_p(0), lambda t: C.c_void_p(t.data_ptr())
    h, stream = mesh._h, capi._stream_ptr()
    for args in ((null, B, d(p), d(a), d(b)), (h, B, null, d(a), d(b)), (h, B, d(p), null, d(b)), (h, 0, d(p), d(a), d(b)), (h, -1, d(p), d(a), d(b)),
                 (h, 2**31 - 1, d(p), d(a), d(b))):  # fmt: skip
        assert L.mmx_vertex_normals(*args, stream) == MMX_ERR_INVALID_ARGUMENT, args
        assert L.mmx_last_error().decode().startswith("mmx_vertex_normals: ")
    for args in ((null, B, d(p), d(b), d(a), d(c)), (h, B, null, d(b), d(a), d(c)), (h, B, d(p), null, d(a), d(c)), (h, B, d(p), d(b), null, d(c)),
                 (h, B, d(p), d(b), d(a), null), (h, 0, d(p), d(b), d(a), d(c)), (h, 2**31 - 1, d(p), d(b), d(a), d(c))):  # fmt: skip
        assert L.mmx_vertex_normals_backward(*args, stream) == MMX_ERR_INVALID_ARGUMENT, args
        assert L.mmx_last_error().decode().startswith("mmx_vertex_normals_backward: ")
    torch.cuda.synchronize()
    assert all(torch.all(t == -7.25).item() for t in (a, b, c))
    with pytest.raises(capi.MmxError):
        capi.Mesh(np.array([[0, 1, V]], np.int32), V)
    # the host forms compute what the device forms do
    cot = ref.cotangent(pos.shape, 83)
    want = _run_gpu(mesh, pos, cot)
    hn, hs, hg = (np.full((B, V, 3), -7.25, np.float32) for _ in range(3))
    hp = lambda x: C.c_void_p(x.ctypes.data)
    tp = capi.as_ptr(np.ascontiguousarray(tri), C.c_int32)
    assert L.mmx_vertex_normals_host(V, len(tri), tp, 0, B, hp(pos), hp(hn), hp(hs)) == 0
    assert np.array_equal(hn, want["normals"]) and np.array_equal(hs, want["sums"])
    hn[:] = -7.25
    assert L.mmx_vertex_normals_host(V, len(tri), tp, 0, B, hp(pos), hp(hn), None) == 0 and np.array_equal(hn, want["normals"])
    assert L.mmx_vertex_normals_backward_host(V, len(tri), tp, 0, B, hp(pos), hp(hs), hp(cot), hp(hg)) == 0
    assert np.array_equal(hg, want["position_grad"])
