"""mmx_closest_points on the GPU against the float64 brute force and the acceptance rule of tests/closest_points_reference.py
(checked on its own, with the float32 restatement, in tests/test_closest_points_reference.py).

The rule, with u = 2^-24: the chosen target's float64 distance is within (1 + 16u) of the nearest eligible target's, dist2 is
within 8u of the chosen target's float64 distance, `valid` is free only where the float64 minimum sits within 16u of
max_dist^2, and with normals the chosen target's dot is at least min_normal_dot - 1e-6 while the minimum is taken over the
targets with dot at least min_normal_dot + 1e-6.  The shapes come from mmx_closest_points_plan (S sources per workgroup, T
targets per tile, W ways): every edge of the kernel, with and without normals, shared and per-instance targets.

Measured on an MI355X (profiles/closest_points_parity.json, written through MMX_PARITY_OUT), the worst over the 56 parity cases
(52 on the unit cloud, 4 on the offset cloud):
    d64(index) / min d64 - 1       0 u      (bound 16 u: every index is a float64 argmin)
    |dist2 - d64(index)| / d64     3.50 u   (bound 8 u)
    indices that differ from the float64 argmin   0;   undecided `valid`   0;   sources with a target in the normal band   0
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import autograd as mauto
from momentum_amd import build as mbuild
from momentum_amd import capi, geometry, make_test_character, make_test_skin
from tests import closest_points_reference as ref
from tests import skeleton_state_reference as fk

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT = 1
INF = float("inf")
_parity = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    """MMX_PARITY_OUT=<file>: the measured figures of this run as JSON (how profiles/closest_points_parity.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _parity:
        worst = {k: max(v[k] for v in _parity.values()) for k in ("worst_ratio_u", "worst_dist2_u", "differ", "undecided", "band")}
        unit = "worst_ratio_u: d64(index) / min d64 - 1 in units of u = 2^-24 (bound 16); worst_dist2_u: |dist2 - d64(index)| / d64(index) in u (bound 8); differ: indices that are not the float64 argmin"
        with open(out, "w") as f:
            json.dump(dict(unit=unit, worst=worst, cases=_parity), f, indent=1)


def _shapes():
    mbuild.build()
    out = []
    for normals in (False, True):
        for B, N, M in ref.parity_shapes(capi.closest_points_plan, normals):
            out += [(B, N, M, normals, shared) for shared in (False, True)]
    return out


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(c, max_dist=INF, min_normal_dot=0.0, **kw):
    """capi.closest_points on a cloud dict -> (index, dist2, points) as numpy (None where not asked for)"""
    res = capi.closest_points(_cuda(c["source"]), _cuda(c["target"]), max_dist, _cuda(c["source_normals"]), _cuda(c["target_normals"]), min_normal_dot, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def _check(c, res, max_dist=INF, min_normal_dot=0.0):
    return ref.check(c["source"], c["target"], res[0], res[1], res[2], max_dist, c["source_normals"], c["target_normals"], min_normal_dot)


@pytest.mark.parametrize("B,N,M,normals,shared", _shapes())
def test_parity(torch_cuda, B, N, M, normals, shared):
    c = ref.cloud("unit", B, N, M, ref.shape_seed(B, N, M, normals, shared), shared, normals)
    mnd = ref.MIN_NORMAL_DOT if normals else 0.0
    s = _check(c, _run(c, min_normal_dot=mnd), min_normal_dot=mnd)
    print(s)
    _parity[f"unit/B{B}_N{N}_M{M}{'_normals' if normals else ''}{'_shared' if shared else ''}"] = s


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_parity_on_the_offset_cloud(torch_cuda, normals, shared):
    """Coordinates 100 +- 0.05: the expanded form |s|^2 + |t|^2 - 2 s.t fails the rule here (tests/test_closest_points_reference.py)."""
    B, N, M = ref.OFFSET_SHAPE
    c = ref.cloud("offset", B, N, M, ref.shape_seed(B, N, M, normals, shared), shared, normals)
    mnd = ref.MIN_NORMAL_DOT if normals else 0.0
    s = _check(c, _run(c, min_normal_dot=mnd), min_normal_dot=mnd)
    print(s)
    _parity[f"offset/B{B}_N{N}_M{M}{'_normals' if normals else ''}{'_shared' if shared else ''}"] = s


@pytest.mark.parametrize("normals", [False, True])
def test_ties_go_to_the_lowest_index(torch_cuda, normals):
    """M0 distinct targets repeated three times: with M0 = T + T/W + 3 the copies of a point fall in different tiles and (a
    wave's share of a tile is T/W targets) in different waves' shares; every index is below M0 and equals the index on the
    first M0 targets."""
    B, N = 2, 70
    p = capi.closest_points_plan(B, N, 3, normals)
    T, W = p["target_tile"], p["target_ways"]
    assert W > 1
    M0 = T + T // W + 3
    c = ref.cloud("unit", B, N, M0, 4242 + normals, True, normals)
    # coarse coordinates: many sources have several DISTINCT targets at exactly equal float32 distance as well
    # (and coarse normals, used as given: every dot is exact, so the threshold falls the same way on both sides)
    for k in c:
        c[k] = None if c[k] is None else (np.round(c[k] * 4) / 4).astype(np.float32)
    first = _run(c, min_normal_dot=-0.5 if normals else 0.0)
    rep = dict(c, target=np.tile(c["target"], (3, 1)), target_normals=None if not normals else np.tile(c["target_normals"], (3, 1)))
    again = _run(rep, min_normal_dot=-0.5 if normals else 0.0)
    assert (again[0] < M0).all() and (again[0] >= 0).all()
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    # ... and the lowest index among equal distances within the M0 targets: the float32 restatement's first minimum, wherever
    # its d2 (no fma) and the kernel's are both exact -- on this grid every term is a multiple of 1/16 below 2^24, so they are
    want, _ = ref.restatement32(c["source"], c["target"], INF, c["source_normals"], c["target_normals"], -0.5)
    assert np.array_equal(first[0], want)


def test_max_dist(torch_cuda):
    c = ref.cloud("unit", 3, 300, 700, 77)
    for max_dist in (0.05, 0.3):
        res = _run(c, max_dist)
        s = _check(c, res, max_dist)
        assert s["undecided"] == 0 and 0 < (res[0] >= 0).sum() < res[0].size, s  # a mix of near and far sources
        none = res[0] < 0
        assert (res[1][none] == np.inf).all() and (res[2][none] == 0).all()
    # max_dist = 0: exactly the sources that coincide with a target are valid
    c["source"][:, ::3] = c["target"][:, 5:105]
    res = _run(c, 0.0)
    hit = np.zeros((3, 300), bool)
    hit[:, ::3] = True
    assert np.array_equal(res[0] >= 0, hit) and np.array_equal(res[0][:, ::3], np.tile(np.arange(5, 105, dtype=np.int32), (3, 1)))
    assert (res[1][hit] == 0).all() and (res[1][~hit] == np.inf).all() and (res[2][~hit] == 0).all()
    assert np.array_equal(res[2][hit], c["source"][hit])
    _check(c, res, 0.0)


@pytest.mark.parametrize("normals", [False, True])
def test_non_finite_inputs(torch_cuda, normals):
    """NaN and infinities are ordinary inputs: a pair with one is ineligible, nothing else changes."""
    B, N, M = 2, 130, 1100
    c = ref.cloud("unit", B, N, M, 99, False, normals)
    mnd = -0.2
    clean = _run(c, min_normal_dot=mnd)
    bad_t = [0, 7, 511, 512, 1023, 1024, 1099]
    dirty = {k: (None if v is None else v.copy()) for k, v in c.items()}
    dirty["source"][0, 5, 1] = np.nan
    dirty["source"][1, 129, 0] = np.inf
    for k, j in enumerate(bad_t):
        dirty["target"][:, j, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    if normals:
        dirty["source_normals"][1, 3, 2] = np.nan
        dirty["target_normals"][:, 20, 0] = np.nan
        bad_t = bad_t + [20]
    res = _run(dirty, min_normal_dot=mnd)
    dead = np.zeros((B, N), bool)
    dead[0, 5] = dead[1, 129] = True
    if normals:
        dead[1, 3] = True
    assert (res[0][dead] == -1).all() and (res[1][dead] == np.inf).all() and (res[2][dead] == 0).all()
    assert (res[0][~dead] >= 0).all() and not np.isin(res[0], bad_t).any() and np.isfinite(res[2]).all()
    _check(dirty, res, min_normal_dot=mnd)  # (the reference drops the same pairs: NaN fails every comparison)
    keep = ~dead & ~np.isin(clean[0], bad_t)
    for a, b in zip(clean, res):
        assert np.array_equal(a[keep], b[keep])
    # an all-NaN target set gives -1 everywhere
    dirty["target"][:] = np.nan
    res = _run(dirty, min_normal_dot=mnd)
    assert (res[0] == -1).all() and (res[1] == np.inf).all() and (res[2] == 0).all()


@pytest.mark.parametrize("normals", [False, True])
def test_shared_target_equals_the_replicated_one(torch_cuda, normals):
    B, N, M = 3, 300, 1500
    c = ref.cloud("unit", B, N, M, 123, True, normals)
    rep = dict(c, target=np.repeat(c["target"][None], B, 0), target_normals=None if not normals else np.repeat(c["target_normals"][None], B, 0))
    for a, b in zip(_run(c, 0.4, 0.1), _run(rep, 0.4, 0.1)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("normals", [False, True])
def test_a_row_depends_on_its_instance_only(torch_cuda, normals):
    c = ref.cloud("unit", 5, 300, 1500, 321, False, normals)
    one = lambda cl, b: {k: (None if v is None else v[b : b + 1]) for k, v in cl.items()}
    alone = _run(one(c, 3), 0.5, 0.1)
    order = [4, 3, 2, 1, 0]
    moved = {k: (None if v is None else v[order]) for k, v in c.items()}
    runs = [_run(c, 0.5, 0.1), _run(moved, 0.5, 0.1), _run(c, 0.5, 0.1)]
    for res, row in zip(runs, (3, 1, 3)):
        for a, b in zip(alone, res):
            assert np.array_equal(a[0].view(np.uint32), b[row].view(np.uint32))


def test_refusals_touch_no_output(torch_cuda):
    B, N, M = 2, 10, 12
    c = ref.cloud("unit", B, N, M, 55, False, True)
    src, tgt, sn, tn = (_cuda(c[k]) for k in ("source", "target", "source_normals", "target_normals"))
    idx = torch.full((B, N), 7, dtype=torch.int32, device="cuda")
    d2 = torch.full((B, N), -7.25, device="cuda")
    pts = torch.full((B, N, 3), -7.25, device="cuda")
    L, stream = capi.lib(), capi._stream_ptr()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok = dict(B=B, N=N, M=M, src=src, tgt=tgt, sn=None, tn=None, max_dist=INF, mnd=0.0, idx=idx)
    bad = [dict(B=0), dict(N=0), dict(M=0), dict(B=-1), dict(src=None), dict(tgt=None), dict(idx=None), dict(max_dist=-0.5), dict(max_dist=float("nan")),
           dict(sn=sn), dict(tn=tn), dict(sn=sn, tn=tn, mnd=float("nan")), dict(B=2**31 - 1, N=2**31 - 1)]  # fmt: skip
    for change in bad:
        a = dict(ok, **change)
        rc = L.mmx_closest_points(a["B"], a["N"], a["M"], p(a["src"]), p(a["tgt"]), 0, p(a["sn"]), p(a["tn"]), a["max_dist"], a["mnd"], p(a["idx"]), p(d2), p(pts), stream)
        assert rc == MMX_ERR_INVALID_ARGUMENT, change
    hi, hd, hp_ = np.full((B, N), 7, np.int32), np.full((B, N), -7.25, np.float32), np.full((B, N, 3), -7.25, np.float32)
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    hok = dict(ok, src=c["source"], tgt=c["target"], idx=hi)
    for change in bad:
        a = dict(hok, **{k: (c["source_normals"] if v is sn else c["target_normals"] if v is tn else v) for k, v in change.items()})
        rc = L.mmx_closest_points_host(a["B"], a["N"], a["M"], hp(a["src"]), hp(a["tgt"]), 0, hp(a["sn"]), hp(a["tn"]), a["max_dist"], a["mnd"], hp(a["idx"]), hp(hd), hp(hp_))
        assert rc == MMX_ERR_INVALID_ARGUMENT, change
    torch.cuda.synchronize()
    assert torch.all(idx == 7).item() and torch.all(d2 == -7.25).item() and torch.all(pts == -7.25).item()
    assert (hi == 7).all() and (hd == -7.25).all() and (hp_ == -7.25).all()
    # nan min_normal_dot is fine without normals (it is not read), and the host form computes what the device form does
    want = _run(dict(c, source_normals=None, target_normals=None), 0.6, float("nan"))
    assert L.mmx_closest_points_host(B, N, M, hp(c["source"]), hp(c["target"]), 0, None, None, 0.6, float("nan"), hp(hi), hp(hd), hp(hp_)) == 0
    assert np.array_equal(hi, want[0]) and np.array_equal(hd, want[1]) and np.array_equal(hp_, want[2])
    want = _run(c, 0.6, 0.2)
    assert L.mmx_closest_points_host(B, N, M, hp(c["source"]), hp(c["target"]), 0, hp(c["source_normals"]), hp(c["target_normals"]), 0.6, 0.2, hp(hi), None, None) == 0
    assert np.array_equal(hi, want[0])


@pytest.mark.parametrize("normals", [False, True])
def test_optional_outputs_do_not_change_the_index(torch_cuda, normals):
    c = ref.cloud("unit", 2, 257, 1030, 66, False, normals)
    full = _run(c, 0.3, 0.1)
    for want_dist2, want_points in ((False, False), (True, False), (False, True)):
        res = _run(c, 0.3, 0.1, want_dist2=want_dist2, want_points=want_points)
        assert np.array_equal(res[0], full[0]) and (res[1] is None) == (not want_dist2) and (res[2] is None) == (not want_points)
        assert res[1] is None or np.array_equal(res[1], full[1])
        assert res[2] is None or np.array_equal(res[2], full[2])


def test_replays_from_a_captured_graph(torch_cuda):
    """After a warm-up call a call is captured into torch.cuda.graph and replayed; the replay reproduces the eager result bit
    for bit.  A capture through the HIP API itself shows the call's graph: one kernel node, no edge (so no parallel branch)."""
    B, N, M = 3, 300, 1500
    clouds = [ref.cloud("unit", B, N, M, s, False, True) for s in (901, 902)]
    eager = [_run(c, 0.5, 0.1) for c in clouds]  # (also the warm-up)
    keys = ("source", "target", "source_normals", "target_normals")
    bufs = {k: _cuda(clouds[0][k]) for k in keys}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = capi.closest_points(bufs["source"], bufs["target"], 0.5, bufs["source_normals"], bufs["target_normals"], 0.1)
    torch.cuda.current_stream().wait_stream(side)
    for k in (0, 1, 0):
        for key in keys:
            bufs[key].copy_(_cuda(clouds[k][key]))
        out[0].fill_(-5)
        out[1].zero_()
        out[2].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager[k]):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), k
    # the graph of one call, through the HIP runtime the library itself is linked against
    L = capi.lib()
    hip_graph, count, edges = C.c_void_p(0), C.c_size_t(0), C.c_size_t(0)
    stream = C.c_void_p(side.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    L.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    assert L.hipStreamBeginCapture(stream, 2) == 0  # hipStreamCaptureModeRelaxed
    rc = L.mmx_closest_points(B, N, M, p(bufs["source"]), p(bufs["target"]), 0, p(bufs["source_normals"]), p(bufs["target_normals"]), 0.5, 0.1,
                              p(out[0]), p(out[1]), p(out[2]), stream)  # fmt: skip
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


def test_find_closest_points_on_skinned_vertices(torch_cuda):
    """geometry.find_closest_points on the output of autograd.skin_points (make_test_skin on the 3-joint character): the ICP
    step without leaving the device."""
    rig = make_test_character(3)
    sk = make_test_skin(rig, 500, 4, 17)
    rh = capi.RigHandle(rig, 0)
    skin = capi.Skin(rh, sk.joint, sk.weight, sk.inverse_bind, sk.rest)
    B = 3
    pb = capi.Problem(rh, B, [0], [])
    pose = lambda seed: mauto.skin_points(skin, pb.skeleton_state(_cuda(np.ascontiguousarray(fk.random_inputs(rig, B, seed)[0], np.float32))))
    verts = pose(5)
    rng = np.random.default_rng(6)
    scan = (pose(7) + _cuda((0.01 * rng.standard_normal((B, 500, 3))).astype(np.float32)))[:, :450].contiguous()
    nearest = (geometry.find_closest_points(verts, scan)[0] - verts).norm(dim=-1)
    for max_dist in (INF, 1.0001 * float(nearest.median())):  # (the second: about half of the vertices have a scan point that near)
        points, index, valid = geometry.find_closest_points(verts, scan, max_dist)
        assert index.dtype == torch.int32 and valid.dtype == torch.bool and points.shape == (B, 500, 3) and not points.requires_grad
        assert torch.equal(valid, index >= 0)
        s = ref.check(verts.cpu().numpy(), scan.cpu().numpy(), index.cpu().numpy(), None, points.cpu().numpy(), max_dist)
        assert s["undecided"] == 0, s
    assert 0 < int(valid.sum()) < valid.numel()
    # the overload with normals, the single-cloud form and the gradient recipe of the docstring
    ns, nt = _cuda(ref.unit_normals(rng, (B, 500))), _cuda(ref.unit_normals(rng, (B, 450)))
    points, index, valid = geometry.find_closest_points(verts, ns, scan, nt, INF, 0.5)
    s = ref.check(verts.cpu().numpy(), scan.cpu().numpy(), index.cpu().numpy(), None, points.cpu().numpy(), INF, ns.cpu().numpy(), nt.cpu().numpy(), 0.5)
    assert s["band"] * 100 <= s["sources"], s
    p1, i1, v1 = geometry.find_closest_points(verts[1], scan[1])
    pb_, ib_, vb_ = geometry.find_closest_points(verts, scan)
    assert torch.equal(p1, pb_[1]) and torch.equal(i1, ib_[1]) and torch.equal(v1, vb_[1])
    tgt = scan.clone().requires_grad_(True)
    gathered = torch.gather(tgt, 1, ib_.long()[..., None].expand(-1, -1, 3))
    assert torch.equal(gathered.detach(), pb_)
    ((gathered - verts) ** 2).sum().backward()
    assert tgt.grad is not None and bool((tgt.grad != 0).any())
