"""mmx_closest_points_on_mesh on the GPU against the float64 brute force and the acceptance rule of
tests/closest_points_on_mesh_reference.py (checked on its own, with the float32 restatement, in
tests/test_closest_points_on_mesh_reference.py).

The rule, with u = 2^-24, R = max(|p - a|, |p - b|, |p - c|) and K = 64 (4 x the restatement's own 9.35 u R, rounded up): the
returned face's float64 distance is within K u (R + R) of the nearest eligible face's, sqrt(dist2) within K u R of the returned
face's float64 distance, the weights are >= 0 and sum to 1 within 4u, the float64 point of the returned weights is within K u R
of optimal, points is a + s e1 + t e2 within two roundings, and `valid` is free only where the float64 minimum sits within
K u R of max_dist.  The shapes come from mmx_closest_points_on_mesh_plan (S sources per workgroup, T_t triangles per tile, W
ways): every edge of the kernel, shared and per-instance vertices.

Measured on an MI355X (profiles/closest_points_on_mesh_parity.json, written through MMX_PARITY_OUT), the worst over the 27
parity cases (26 shapes at the origin, 1 on the mesh at offset 100), bound K = 64 each (the float32 restatement itself: 9.35):
    (d64(f) - min d64) / (R + R)         0.28 u
    |sqrt(dist2) - d64(f)| / R           9.07 u
    point of the weights, from optimal   8.98 u R
    |w_a + w_b + w_c - 1|                0 u      (bound 4 u: the weights are multiples of 2^-24 and sum to 1 exactly)
    undecided `valid`                    0
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import autograd as mauto
from momentum_amd import build as mbuild
from momentum_amd import capi, geometry, make_humanoid72, make_test_character
from momentum_amd.rigs import make_test_skinned_mesh
from tests import closest_points_on_mesh_reference as ref
from tests import skeleton_state_reference as fk
from tests import skinning_reference as skin_ref

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT = 1
INF = float("inf")
FIGURES = ("worst_choice", "worst_dist", "worst_weights", "worst_sum_u", "undecided")
_parity = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    """MMX_PARITY_OUT=<file>: the measured figures of this run as JSON (how profiles/closest_points_on_mesh_parity.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _parity:
        worst = {k: max(v[k] for v in _parity.values()) for k in FIGURES}
        unit = ("worst_choice: (d64(p, f) - min d64) / (R(p, f) + R(p, g*)); worst_dist: |sqrt(dist2) - d64(p, f)| / R; worst_weights: | |sum(w vertex) - p| - d64(p, f)| / R, "
                "all in units of u = 2^-24 (bound K = %d); worst_sum_u: |w_a + w_b + w_c - 1| in u (bound 4)" % ref.K)  # fmt: skip
        with open(out, "w") as f:
            json.dump(dict(unit=unit, K=ref.K, worst=worst, cases=_parity), f, indent=1)


def _shapes():
    mbuild.build()
    return [(B, N, T, shared) for B, N, T in ref.parity_shapes(capi.closest_points_on_mesh_plan) for shared in (False, True)]


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


_meshes = {}


def _mesh(tri, V):
    """a handle per (triangle list, V), kept for the module"""
    key = (np.asarray(tri, np.int32).tobytes(), int(V))
    if key not in _meshes:
        _meshes[key] = capi.Mesh(np.asarray(tri, np.int32), int(V))
    return _meshes[key]


def _run(c, max_dist=INF, **kw):
    """Mesh.closest_points on a case dict -> (face, barycentric, points, dist2) as numpy (None where not asked for)"""
    kw.setdefault("want_dist2", True)
    res = _mesh(c["triangles"], c["vertices"].shape[-2]).closest_points(_cuda(c["source"]), _cuda(c["vertices"]), max_dist, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def _check(c, res, max_dist=INF, triangles=None):
    return ref.check(c["source"], c["vertices"], c["triangles"] if triangles is None else triangles, res[0], res[1], res[2], res[3], max_dist)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("B,N,T,shared", _shapes())
def test_parity(torch_cuda, B, N, T, shared):
    c = ref.parity_case(B, N, T, shared)
    s = _check(c, _run(c))
    print(s)
    assert s["valid"] == s["sources"]
    _parity[f"origin/B{B}_N{N}_T{T}{'_shared' if shared else ''}"] = s


def test_parity_on_the_offset_mesh(torch_cuda):
    """The mesh at (100, 100, 100): with differences taken first every error is relative to R, not to the coordinates."""
    B, N, T = ref.OFFSET_SHAPE
    c = ref.parity_case(B, N, T, False, offset=(100.0, 100.0, 100.0))
    s = _check(c, _run(c))
    print(s)
    assert s["valid"] == s["sources"]
    _parity[f"offset/B{B}_N{N}_T{T}"] = s


def test_ties_go_to_the_lowest_face(torch_cuda):
    """T0 triangles repeated three times: with T0 = T_t + T_t / W + 3 the copies of a triangle fall in different tiles and in
    different waves' shares; every face index is below T0 and every output equals the unrepeated run bit for bit."""
    B, N = 2, 70
    p = capi.closest_points_on_mesh_plan(B, N, 3)
    Tt, W = p["triangle_tile"], p["triangle_ways"]
    T0 = Tt + Tt // W + 3
    c = ref.parity_case(B, N, T0, False)
    first = _run(c)
    again = _run(dict(c, triangles=np.tile(c["triangles"], (3, 1))))
    assert (again[0] < T0).all() and (again[0] >= 0).all()
    assert _same_bits(first, again)
    # a mesh and sources on multiples of 1/4 (a grid of unit right triangles, so that the reciprocals 1, 1, 1/2 and 1 of the
    # record are exact too): every float32 operation of the pair is exact with or without fma, many sources are equally near
    # several faces, and the face is the restatement's first minimum
    n = 13
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vtx = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3).astype(np.float32)
    at = lambda i, j: (i * n + j).reshape(-1)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    tri = np.stack([np.stack([at(i, j), at(i + 1, j), at(i, j + 1)], 1), np.stack([at(i + 1, j + 1), at(i, j + 1), at(i + 1, j)], 1)], 1).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32)  # (288 triangles: more than a tile)
    assert tri.shape[0] > Tt
    rng = np.random.default_rng(5)
    src = (np.round(rng.uniform(-1, n, (B, 200, 3)) * 4) / 4).astype(np.float32)
    src[..., 2] = np.round(rng.uniform(-1, 1, (B, 200)) * 4) / 4
    g = dict(source=src, vertices=vtx, triangles=tri)
    got = _run(g)
    want = ref.restatement32(src, vtx, tri)
    d2 = ref.triangle_math(src, vtx, tri, np.float32)[2]
    assert ((d2 == d2.min(-1, keepdims=True)).sum(-1) > 1).mean() > 0.2  # ties are common here
    assert np.array_equal(got[0], want[0]) and _same_bits(got[1:], want[1:])
    rep = _run(dict(g, triangles=np.tile(tri, (3, 1))))
    assert _same_bits(got, rep)


def test_max_dist(torch_cuda):
    B, N, T = ref.MAX_DIST_SHAPE
    c = ref.parity_case(B, N, T, False)
    for max_dist in ref.MAX_DIST_VALUES:
        res = _run(c, max_dist)
        s = _check(c, res, max_dist)
        assert s["undecided"] == 0 and 0 < s["valid"] < s["sources"], s  # a mix of valid and invalid sources
        none = res[0] < 0
        assert (res[1][none] == 0).all() and (res[2][none] == 0).all() and (res[3][none] == np.inf).all()
    # max_dist = 0: exactly the sources that are bitwise a vertex of an eligible face are valid.  Every third source becomes a
    # vertex of the instance's mesh; the others are the mix's sources at normal noise 0.02 and 0.3 (a source ON the surface
    # may round to a residual of exact zeros, which is a valid result too)
    used = np.unique(c["triangles"])
    src = c["source"].copy()
    far = np.arange(N) % 4 >= 2
    src[:, ~far] = src[:, far]
    hit = np.zeros((B, N), bool)
    hit[:, ::3] = True
    pick = used[(7 * np.arange(hit[0].sum())) % len(used)]
    src[:, ::3] = c["vertices"][:, pick]
    z = dict(c, source=src)
    res = _run(z, 0.0)
    assert np.array_equal(res[0] >= 0, hit)
    assert (res[3][hit] == 0).all() and (res[3][~hit] == np.inf).all() and (res[1][~hit] == 0).all() and (res[2][~hit] == 0).all()
    # (points is a + s e1 + t e2 from the record: at corner b that is a + (b - a), the vertex within a rounding -- ref.check below)
    assert ((res[1][hit] == 1).sum(-1) == 1).all() and ((res[1][hit] == 0).sum(-1) == 2).all()  # one weight 1, two 0
    corner = c["triangles"][res[0][hit], res[1][hit].argmax(-1)]
    assert np.array_equal(corner, np.tile(pick, B))
    ref.check(src[:, ::3].copy(), c["vertices"], c["triangles"], res[0][:, ::3].copy(), res[1][:, ::3].copy(), res[2][:, ::3].copy(), res[3][:, ::3].copy(), 0.0)


def test_non_finite_inputs(torch_cuda):
    """NaN and infinities are ordinary inputs: a face with a NaN vertex is ineligible for every source, a non-finite source gets
    -1, nothing else changes."""
    B, N, T = 2, 130, 300
    c = ref.parity_case(B, N, T, False)
    clean = _run(c)
    dirty = {k: v.copy() for k, v in c.items()}
    dirty["source"][0, 5, 1] = np.nan
    dirty["source"][1, 129, 0] = np.inf
    bad_vertex = int(c["triangles"][40, 1])
    dirty["vertices"][:, bad_vertex, 2] = np.nan
    bad_faces = np.nonzero((c["triangles"] == bad_vertex).any(1))[0]
    assert 1 < len(bad_faces) < 8
    # sources right above the faces of the NaN vertex: they get the next-nearest face
    mid = c["vertices"][:, c["triangles"][bad_faces]].mean(2)  # [B, F, 3]
    dirty["source"][:, 10 : 10 + len(bad_faces)] = mid
    res = _run(dirty)
    dead = np.zeros((B, N), bool)
    dead[0, 5] = dead[1, 129] = True
    assert (res[0][dead] == -1).all() and (res[1][dead] == 0).all() and (res[2][dead] == 0).all() and (res[3][dead] == np.inf).all()
    assert (res[0][~dead] >= 0).all() and not np.isin(res[0], bad_faces).any() and np.isfinite(res[2]).all()
    # the rule against the reference with those faces removed (indices remapped)
    keep = np.setdiff1d(np.arange(T), bad_faces)
    remap = np.full(T + 1, -1, np.int32)
    remap[keep] = np.arange(len(keep), dtype=np.int32)
    live = dict(dirty, vertices=np.nan_to_num(dirty["vertices"], nan=0.0))  # (the vertex is unused once its faces are gone)
    ref.check(live["source"], live["vertices"], c["triangles"][keep], remap[res[0]], res[1], res[2], res[3])
    _check(dirty, res)  # ... and with them in: the reference drops the same faces
    same = ~dead & ~np.isin(clean[0], bad_faces)
    same[:, 10 : 10 + len(bad_faces)] = False
    for a, b in zip(clean, res):
        assert np.array_equal(a[same], b[same])
    # a mesh of only NaN vertices gives -1 everywhere
    dirty["vertices"][:] = np.nan
    res = _run(dirty)
    assert (res[0] == -1).all() and (res[1] == 0).all() and (res[2] == 0).all() and (res[3] == np.inf).all()


def test_degenerate_faces_are_never_returned(torch_cuda):
    B, N, T = 2, 130, 300
    c = ref.parity_case(B, N, T, True)
    base = _run(c)
    # repeated-vertex triangles at known indices: (a, a, b), (a, b, a), (a, b, b), (a, a, a)
    at = np.array([0, 1, 63, 64, 255, 256, 257, 300, 301, 307])  # positions in the new list (first, tile and wave-share edges, last)
    tri, k = [], 0
    forms = ([0, 0, 1], [0, 1, 0], [0, 1, 1], [0, 0, 0])
    for i in range(T + len(at)):
        if i in at:
            tri.append(c["triangles"][(13 * i) % T][forms[i % 4]])
        else:
            tri.append(c["triangles"][k])
            k += 1
    tri = np.asarray(tri, np.int32)
    assert k == T
    good = np.setdiff1d(np.arange(len(tri)), at)
    res = _run(dict(c, triangles=tri))
    assert not np.isin(res[0], at).any() and (res[0] >= 0).all()
    remap = np.full(len(tri), -1, np.int32)
    remap[good] = np.arange(T, dtype=np.int32)
    assert np.array_equal(remap[res[0]], base[0]) and _same_bits(res[1:], base[1:])
    _check(dict(c, triangles=tri), res)
    res = _run(dict(c, triangles=tri[at]))  # a mesh of only degenerate faces
    assert (res[0] == -1).all() and (res[1] == 0).all() and (res[2] == 0).all() and (res[3] == np.inf).all()


def test_shared_vertices_equal_the_replicated_ones(torch_cuda):
    B, N, T = 3, 300, 520
    c = ref.parity_case(B, N, T, True)
    rep = dict(c, vertices=np.repeat(c["vertices"][None], B, 0))
    for md in (INF, 0.01):
        assert _same_bits(_run(c, md), _run(rep, md))


def test_a_row_depends_on_its_instance_only(torch_cuda):
    c = ref.parity_case(5, 300, 520, False)
    one = lambda cl, b: dict(cl, source=cl["source"][b : b + 1], vertices=cl["vertices"][b : b + 1])
    alone = _run(one(c, 3), 0.05)
    order = [4, 3, 2, 1, 0]
    moved = dict(c, source=c["source"][order], vertices=c["vertices"][order])
    runs = [_run(c, 0.05), _run(moved, 0.05), _run(c, 0.05)]
    for res, row in zip(runs, (3, 1, 3)):
        for a, b in zip(alone, res):
            assert np.array_equal(a[0].view(np.uint32), b[row].view(np.uint32))
    assert _same_bits(runs[0], runs[2])


def test_optional_outputs_do_not_change_the_others(torch_cuda):
    c = ref.parity_case(2, 257, 300, False)
    full = _run(c, 0.05)
    for wb, wp, wd in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        res = _run(c, 0.05, want_barycentric=wb, want_points=wp, want_dist2=wd)
        assert [r is not None for r in res] == [True, wb, wp, wd]
        assert all(r is None or np.array_equal(r, f) for r, f in zip(res, full))


def test_refusals_touch_no_output(torch_cuda):
    B, N, T = 2, 10, 12
    c = ref.parity_case(B, N, T, False)
    V = c["vertices"].shape[1]
    mesh = _mesh(c["triangles"], V)
    src, vtx = _cuda(c["source"]), _cuda(c["vertices"])
    face = torch.full((B, N), 7, dtype=torch.int32, device="cuda")
    bary, pts, d2 = (torch.full(s, -7.25, device="cuda") for s in ((B, N, 3), (B, N, 3), (B, N)))
    L, stream = capi.lib(), capi._stream_ptr()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok = dict(mesh=mesh._h, B=B, N=N, src=src, vtx=vtx, max_dist=INF, face=face)
    bad = [dict(mesh=None), dict(B=0), dict(N=0), dict(B=-1), dict(src=None), dict(vtx=None), dict(face=None), dict(max_dist=-0.5),
           dict(max_dist=float("nan")), dict(B=2**31 - 1, N=2**31 - 1)]  # fmt: skip
    for change in bad:
        a = dict(ok, **change)
        rc = L.mmx_closest_points_on_mesh(a["mesh"], a["B"], a["N"], p(a["src"]), p(a["vtx"]), 0, a["max_dist"], p(a["face"]), p(bary), p(pts), p(d2), stream)
        assert rc == MMX_ERR_INVALID_ARGUMENT and L.mmx_last_error().decode().startswith("mmx_closest_points_on_mesh: "), change
    torch.cuda.synchronize()
    assert torch.all(face == 7).item() and all(torch.all(t == -7.25).item() for t in (bary, pts, d2))
    # the host form computes what the device form does
    want = _run(c, 0.05)
    hf, hb, hp_, hd = np.full((B, N), 7, np.int32), np.zeros((B, N, 3), np.float32), np.zeros((B, N, 3), np.float32), np.zeros((B, N), np.float32)
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    tri = np.ascontiguousarray(c["triangles"], np.int32)
    rc = L.mmx_closest_points_on_mesh_host(V, T, tri.ctypes.data_as(C.POINTER(C.c_int32)), 0, B, N, hp(c["source"]), hp(c["vertices"]), 0, 0.05,
                                           hp(hf), hp(hb), hp(hp_), hp(hd))  # fmt: skip
    assert rc == 0 and _same_bits((hf, hb, hp_, hd), want)
    rc = L.mmx_closest_points_on_mesh_host(V, T, tri.ctypes.data_as(C.POINTER(C.c_int32)), 0, B, N, hp(c["source"]), hp(c["vertices"]), 0, 0.05,
                                           hp(hf), None, None, None)  # fmt: skip
    assert rc == 0 and np.array_equal(hf, want[0])


def test_replays_from_a_captured_graph(torch_cuda):
    """After a warm-up call a call is captured into torch.cuda.graph and replayed twice on changed inputs; the replay reproduces
    the eager result bit for bit.  A capture through the HIP API itself shows the call's graph: one kernel node, no edge."""
    B, N, T = 3, 300, 520
    cases = [ref.parity_case(B, N, T, False), ref.parity_case(B, N + 0, T, False)]
    cases[1] = dict(cases[1], source=cases[1]["source"][:, ::-1].copy(), vertices=(cases[1]["vertices"] * np.float32(1.01)))
    eager = [_run(c, 0.05) for c in cases]  # (also the warm-up)
    mesh = _mesh(cases[0]["triangles"], cases[0]["vertices"].shape[1])
    bufs = {k: _cuda(cases[0][k]) for k in ("source", "vertices")}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = mesh.closest_points(bufs["source"], bufs["vertices"], 0.05, want_dist2=True)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 0):
        for key in bufs:
            bufs[key].copy_(_cuda(cases[k][key]))
        out[0].fill_(-5)
        for t in out[1:]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits([t.cpu().numpy() for t in out], eager[k]), k
    # the graph of one call, through the HIP runtime the library itself is linked against
    L = capi.lib()
    hip_graph, count, edges = C.c_void_p(0), C.c_size_t(0), C.c_size_t(0)
    stream = C.c_void_p(side.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    L.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    assert L.hipStreamBeginCapture(stream, 2) == 0  # hipStreamCaptureModeRelaxed
    rc = L.mmx_closest_points_on_mesh(mesh._h, B, N, p(bufs["source"]), p(bufs["vertices"]), 0, 0.05, p(out[0]), p(out[1]), p(out[2]), p(out[3]), stream)
    L.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    assert L.hipStreamEndCapture(stream, C.byref(hip_graph)) == 0 and rc == 0 and hip_graph.value
    L.hipGraphGetNodes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    assert L.hipGraphGetNodes(hip_graph, None, C.byref(count)) == 0 and count.value == 1, count.value
    node, kind = C.c_void_p(0), C.c_int(-1)
    assert L.hipGraphGetNodes(hip_graph, C.byref(node), C.byref(count)) == 0
    L.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert L.hipGraphNodeGetType(node, C.byref(kind)) == 0 and kind.value == 0  # hipGraphNodeTypeKernel
    L.hipGraphGetEdges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    assert L.hipGraphGetEdges(hip_graph, None, None, C.byref(edges)) == 0 and edges.value == 0
    L.hipGraphDestroy.argtypes = [C.c_void_p]
    assert L.hipGraphDestroy(hip_graph) == 0


def _dist(x, x64):
    x, x64 = x.reshape(x.shape[0], -1), x64.reshape(x64.shape[0], -1)
    scale = np.abs(x64).max(axis=1)
    return np.abs(x.astype(np.float64) - x64).max(axis=1) / np.where(scale > 0, scale, 1.0)


@pytest.mark.parametrize("rig_name", ["character3", "humanoid72"])
def test_composition_with_skinning_backpropagates_to_theta(torch_cuda, rig_name):
    """theta -> skeleton_state -> skin_points -> find_closest_points_on_mesh on the skin's own triangles; the barycentrics are
    recombined in torch and sum |p - q|^2 is backpropagated to theta.  dL/dtheta is finite and agrees with the float64 torch
    reference of the same fixed faces and weights to the tolerance tests/test_gpu_skin_points.py uses through both stages:
    4 x the distance of the float32 torch reference from the float64 one."""
    rig = make_test_character(3) if rig_name == "character3" else make_humanoid72(variant="p128", unit=0.01)
    sk, tri = make_test_skinned_mesh(rig, 12, 8, 4, 91)
    V, B, N = sk.rest.shape[0], 3, 150
    rh = capi.RigHandle(rig, 0)
    skin = capi.Skin(rh, sk.joint, sk.weight, sk.inverse_bind, sk.rest)
    mesh = capi.Mesh(tri, V)
    pb = capi.Problem(rh, B, [0], [])
    theta, _ = fk.random_inputs(rig, B, seed=92)
    th = _cuda(np.ascontiguousarray(theta, np.float32)).requires_grad_(True)
    verts = mauto.skin_points(skin, mauto.skeleton_state(pb, th))
    # the scan: points of the posed surface of ANOTHER pose, with noise
    other = mauto.skin_points(skin, pb.skeleton_state(_cuda(np.ascontiguousarray(fk.random_inputs(rig, B, seed=93)[0], np.float32)))).cpu().numpy()
    scale = float(np.abs(sk.rest).max())
    scan_np = ref.source_mix(other, tri, B, N, 94, noises=tuple(scale * x for x in ref.NOISES))
    scan = _cuda(scan_np)
    valid, closest, face, bary = geometry.find_closest_points_on_mesh(scan, verts, mesh)
    assert valid.dtype == torch.bool and face.dtype == torch.int32 and not closest.requires_grad and not bary.requires_grad and bool(valid.all())
    ref.check(scan_np, verts.detach().cpu().numpy(), tri, face.cpu().numpy(), bary.cpu().numpy(), closest.cpu().numpy())
    faces = torch.as_tensor(tri.astype(np.int64)).cuda()
    bidx = torch.arange(B, device="cuda")[:, None]
    q = (bary[..., None] * verts[bidx[..., None], faces[face.long()]]).sum(-2)  # the docstring's recombination
    assert torch.allclose(q.detach(), closest, rtol=0, atol=4 * ref.U * scale * 4)
    ((scan - q) ** 2).sum().backward()
    got = th.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got).max() > 0

    def chain(dtype):
        rt = fk.RigTensors(rig, dtype)
        st = skin_ref.SkinTensors(sk.joint, sk.weight, sk.inverse_bind, sk.rest, rig.num_joints, dtype)
        x = torch.as_tensor(theta, dtype=dtype).clone().requires_grad_(True)
        v = skin_ref.skin_points(st, fk.skeleton_state(rt, x))
        w = torch.as_tensor(bary.cpu().numpy(), dtype=dtype)
        f = torch.as_tensor(tri.astype(np.int64))[torch.as_tensor(face.cpu().numpy()).long()]
        qq = (w[..., None] * v[torch.arange(B)[:, None, None], f]).sum(-2)
        ((torch.as_tensor(scan_np, dtype=dtype) - qq) ** 2).sum().backward()
        return x.grad.numpy()

    want64, want32 = chain(torch.float64), chain(torch.float32)
    d32, dg = _dist(want32, want64), _dist(got, want64)
    print(f"composition_{rig_name}: theta_grad gpu {dg.max():.3e}  d32 {d32.max():.3e}  bound {4 * d32.max():.3e}")
    assert dg.max() <= 4 * d32.max(), (dg, d32)
    mesh.close()


def test_find_closest_points_on_mesh_call_shapes(torch_cuda):
    """(valid, closest_points, face_index, barycentric); valid is bool, face_index int32; the [N, 3] form; a capi.Mesh, a tensor
    or an array as faces_target; max_dist is keyword-only."""
    B, N, T = 2, 90, 300
    c = ref.parity_case(B, N, T, False)
    src, vtx = _cuda(c["source"]), _cuda(c["vertices"])
    want = _run(c, want_dist2=False)
    mesh = _mesh(c["triangles"], c["vertices"].shape[1])
    for faces in (mesh, torch.from_numpy(c["triangles"].astype(np.int64)).cuda(), torch.from_numpy(c["triangles"]), c["triangles"]):
        valid, closest, face, bary = geometry.find_closest_points_on_mesh(src, vtx, faces)
        assert valid.dtype == torch.bool and face.dtype == torch.int32 and closest.dtype == bary.dtype == torch.float32
        assert valid.shape == face.shape == (B, N) and closest.shape == bary.shape == (B, N, 3)
        assert torch.equal(valid, face >= 0) and _same_bits([t.cpu().numpy() for t in (face, bary, closest)], want[:3])
    v1, c1, f1, b1 = geometry.find_closest_points_on_mesh(src[1], vtx[1], mesh)  # [N, 3] sources, [V, 3] vertices
    assert v1.shape == (N,) and c1.shape == (N, 3) and torch.equal(f1, face[1]) and torch.equal(b1, bary[1]) and torch.equal(c1, closest[1])
    valid, closest, face, bary = geometry.find_closest_points_on_mesh(src, vtx, mesh, max_dist=ref.MAX_DIST_VALUES[0])
    assert 0 < int(valid.sum()) < valid.numel() and bool((closest[~valid] == 0).all()) and bool((face[~valid] == -1).all())
    with pytest.raises(TypeError):
        geometry.find_closest_points_on_mesh(src, vtx, mesh, 0.5)
    g = vtx.clone().requires_grad_(True)
    out = geometry.find_closest_points_on_mesh(src, g, mesh)
    assert all(not t.requires_grad for t in out)
