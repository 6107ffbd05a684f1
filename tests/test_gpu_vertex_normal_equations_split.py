"""mmx_skin_normal_equations_split on the GPU: an instance's 32-row tiles divided over `parts` workgroups, the partial results
added in a fixed order by a second kernel (include/mmx.h).

What is exact is tested exactly: parts 1 is the unsplit call; where every part boundary is a constraint boundary, H is
float32 of the float64 running sum (parts ascending) of the unsplit kernel's H on the constraint slices; parts >= T is parts = T;
bits depend on the instance and the effective parts only; the workspace's prior contents reach nothing.

g and err cannot be rebuilt from rounded outputs; against the unsplit call on the whole set, per instance
    max|g - g1| <= 2^-23 max|g1|     (both are one float32 rounding of double sums that differ only in association)
    |err - err1| <= 2^-40 err1       (terms at most 4096, non-negative, summed in double: C 2^-53)
Where a part boundary cuts a position constraint the parts are no slices, and the results meet the float64 reference of
tests/vertex_constraints_reference.py within the bound of tests/test_gpu_vertex_normal_equations.py and nothing new:
max(4 x the distance of the same reference run in float32, 16 x 2^-24), distance = per instance max|X - X64| / max|X64|.

Measured on an MI355X (largest distance over the instances: gpu | d32 | bound; profiles/skin_normal_equations_split_parity.json,
written through MMX_PARITY_OUT):
    position_c22/parts2         H 1.89e-07 | 2.57e-07 | 1.03e-06   g 1.06e-07 | 5.08e-07 | 2.03e-06   err 7.02e-09 | 5.24e-07 | 2.10e-06
    position_c22/parts3         H 2.46e-07 | 2.57e-07 | 1.03e-06   g 1.06e-07 | 5.08e-07 | 2.03e-06   err 7.02e-09 | 5.24e-07 | 2.10e-06
    position_c11/parts2         H 2.26e-07 | 3.99e-07 | 1.59e-06   g 1.21e-07 | 6.52e-07 | 2.61e-06   err 8.41e-08 | 6.47e-07 | 2.59e-06
    humanoid_triangles/parts2   H 1.13e-07 | 2.15e-07 | 9.54e-07   g 7.41e-08 | 2.53e-07 | 1.01e-06   err 4.35e-08 | 5.57e-08 | 9.54e-07
    humanoid_triangles/parts5   H 8.78e-08 | 2.15e-07 | 9.54e-07   g 7.41e-08 | 2.53e-07 | 1.01e-06   err 4.35e-08 | 5.57e-08 | 9.54e-07
    humanoid_triangles/parts19  H 6.76e-08 | 2.15e-07 | 9.54e-07   g 7.41e-08 | 2.53e-07 | 1.01e-06   err 4.35e-08 | 5.57e-08 | 9.54e-07
    humanoid_triangles/parts512 H 6.76e-08 | 2.15e-07 | 9.54e-07   g 7.41e-08 | 2.53e-07 | 1.01e-06   err 4.35e-08 | 5.57e-08 | 9.54e-07
    k8/parts3                   H 2.39e-07 | 7.69e-07 | 3.08e-06   g 2.09e-07 | 4.14e-07 | 1.65e-06   err 1.73e-07 | 1.13e-07 | 9.54e-07
    k8_c100/parts3              H 1.56e-07 | 4.92e-07 | 1.97e-06   g 6.14e-08 | 4.06e-07 | 1.63e-06   err 3.76e-08 | 1.60e-07 | 9.54e-07
    random_tree/parts3          H 4.28e-07 | 4.32e-07 | 1.73e-06   g 2.04e-07 | 2.07e-07 | 9.54e-07   err 9.22e-08 | 8.85e-08 | 9.54e-07
    instance_rest/parts3        H 3.08e-07 | 6.98e-07 | 2.79e-06   g 1.09e-07 | 3.89e-07 | 1.55e-06   err 9.81e-08 | 6.66e-08 | 9.54e-07
    enabled_mask_n5/parts3      H 2.56e-08 | 4.88e-08 | 9.54e-07   g 9.84e-08 | 1.79e-07 | 9.54e-07   err 2.58e-08 | 1.94e-08 | 9.54e-07
    enabled_mask_n33/parts3     H 4.46e-08 | 1.13e-07 | 9.54e-07   g 9.84e-08 | 1.79e-07 | 9.54e-07   err 2.58e-08 | 1.94e-08 | 9.54e-07
    skipped_s1/parts2           H 3.26e-07 | 3.21e-07 | 1.29e-06   g 8.93e-08 | 2.55e-07 | 1.02e-06   err 9.61e-08 | 1.09e-07 | 9.54e-07
    skipped_s3/parts2           H 3.63e-07 | 3.82e-07 | 1.53e-06   g 1.40e-07 | 2.49e-07 | 9.97e-07   err 6.97e-08 | 8.99e-08 | 9.54e-07
    gn_fit/parts1               theta 1.26e-05 | 1.73e-05 | 6.94e-05
    gn_fit/parts4               theta 2.91e-05 | 1.73e-05 | 6.94e-05
Every figure is inside its bound (the largest share of a bound: 0.42).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import _abi
from momentum_amd import capi, geometry, make_humanoid72, make_test_character, make_test_skin
from tests import skeleton_state_reference as fk
from tests import skinning_reference as skr
from tests import vertex_constraints_reference as vcr

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT, MMX_ERR_UNSUPPORTED = 1, 4
FLOOR = 16 * 2.0**-24
_parity = {}
_cases, _problems, _refs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    """MMX_PARITY_OUT=<file>: the measured distances of this run as JSON.  Problems and skins are closed before their rigs."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _parity:
        unit = "per instance max|X - X_ref64| / max|X_ref64| (err: relative), largest over the instances; bound = max(4 x d32, 16 x 2^-24)"
        with open(out, "w") as f:
            json.dump(dict(unit=unit, shapes=_parity), f, indent=1)
    for pb in _problems.values():
        pb.close()
    _problems.clear()
    for case in _cases.values():
        case.close()
    _cases.clear()


def _cuda(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


class Case:
    """A rig and a skin on it (arrays and device handle)."""

    def __init__(self, rig, joint, weight, inverse_bind, rest):
        self.rig = rig
        self.arrays = (np.asarray(joint, np.int32), np.asarray(weight, np.float32), inverse_bind, np.asarray(rest, np.float32))
        self.rh = capi.RigHandle(rig, 0)
        self.skin = capi.Skin(self.rh, *self.arrays)
        self.V, self.K = self.arrays[0].shape

    @classmethod
    def synthetic(cls, rig, V, K, seed, random_affine=False):
        s = make_test_skin(rig, V, K, seed, random_affine)
        return cls(rig, s.joint, s.weight, s.inverse_bind, s.rest)

    def theta(self, B, seed):
        return fk.random_inputs(self.rig, B, seed)[0]

    def close(self):
        self.skin.close()
        self.rh.close()

    def reference(self, theta, con, dtype, **kw):
        return vcr.normal_equations(self.rig, self.arrays, theta, con, dtype=dtype, **kw)


def _random_tree():
    rig = fk.all_dofs_rig(fk.random_tree(9, 3), seed=4)  # every dof of every joint: P = 63, scales included
    rig.pt_offsets = np.random.default_rng(5).uniform(-0.2, 0.2, size=7 * rig.num_joints).astype(np.float32)
    return Case.synthetic(rig, 40, 3, 6, True)


def _case(name):
    if name not in _cases:
        _cases[name] = dict(
            character24=lambda: Case.synthetic(make_test_character(24), 80, 2, 61, True),
            humanoid=lambda: Case.synthetic(make_humanoid72(variant="p128", unit=0.01), 300, 4, 42),
            random_tree=_random_tree,
            k8=lambda: Case.synthetic(make_test_character(24), 60, 8, 63, True),
        )[name]()
    return _cases[name]


def _problem(cname, B, enabled=None):
    """One problem per (rig, batch, mask) for the module (closed in _teardown, before the rigs)."""
    key = (cname, B, None if enabled is None else enabled.tobytes())
    if key not in _problems:
        pb = capi.Problem(_case(cname).rh, B, [0], [])  # (the position constraint on the root is never given data: it is not read)
        if enabled is not None:
            pb.set_enabled(enabled)
        _problems[key] = pb
    return _problems[key]


def _constraints(V, B, Cn, S, plane, seed, fw=0.7):
    rng = np.random.default_rng(seed)
    vertex = rng.integers(0, V, size=(B, Cn, S)).astype(np.int32)
    bary = rng.dirichlet(np.ones(3), size=(B, Cn)).astype(np.float32) if S == 3 else None
    normal = rng.normal(size=(B, Cn, 3)).astype(np.float32) if plane else None
    target = rng.normal(scale=0.5, size=(B, Cn, 3)).astype(np.float32)
    return vcr.Constraints(target, vertex, bary, normal, rng.uniform(0.5, 2.0, size=(B, Cn)).astype(np.float32), fw)


def _slice(con, c0, c1, rows=slice(None)):
    cut = lambda a: None if a is None else np.ascontiguousarray(a[rows, c0:c1])
    return vcr.Constraints(cut(con.target), cut(con.vertex), cut(con.barycentric), cut(con.normal), cut(con.weight), con.fw)


def _tiles(con):
    return -(-(con.C if con.normal is not None else 3 * con.C) // 32)


def _run(pb, skin, theta, con, parts=None, rest=None, want=("jtj", "jtr", "err"), workspace="exact", fill=None):
    """parts None: the unsplit call (Problem.vertex_normal_equations as it always was).  Else mmx_skin_normal_equations_split
    itself: workspace "exact" = a fresh tensor of exactly the reported size (filled with the byte `fill` if given), None = a
    null pointer, or a tensor."""
    cpu = lambda t: None if t is None else t.cpu().numpy()
    if parts is None:
        vertex = _cuda(con.vertex[..., 0] if con.S == 1 else con.vertex, np.int32)
        H, g, e = pb.vertex_normal_equations(
            skin, _cuda(theta), _cuda(con.target), vertex=vertex, barycentric=_cuda(con.barycentric), normal=_cuda(con.normal),
            weight=_cuda(con.weight), rest=_cuda(rest), function_weight=con.fw, want=want,
        )  # fmt: skip
        torch.cuda.synchronize()
        return dict(H=cpu(H), g=cpu(g), err=cpu(e))
    B, n = pb.B, pb.n
    dev = [_cuda(con.vertex, np.int32), _cuda(con.barycentric), _cuda(con.target), _cuda(con.normal), _cuda(con.weight), _cuda(rest)]
    th = _cuda(theta)
    H = torch.empty((B, n, n), device="cuda") if "jtj" in want else None
    g = torch.empty((B, n), device="cuda") if "jtr" in want else None
    e = torch.empty((B,), dtype=torch.float64, device="cuda") if "err" in want else None
    if isinstance(workspace, str):
        need = capi.skin_normal_equations_workspace_bytes(B, n, parts)
        assert need >= 0
        workspace = torch.empty((need,), dtype=torch.uint8, device="cuda") if need > 0 else None
        if workspace is not None and fill is not None:
            workspace.fill_(fill)
    ptr = lambda t: None if t is None else t.data_ptr()
    d = _abi.VertexConstraints(_abi.MMX_VC_PLANE if con.normal is not None else _abi.MMX_VC_POSITION, con.C, con.S, con.fw, *(ptr(t) for t in dev))
    rc = capi.lib().mmx_skin_normal_equations_split(
        pb._h, skin._h, C.byref(d), ptr(th), ptr(H), ptr(g), ptr(e), parts, ptr(workspace), 0 if workspace is None else workspace.numel(),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))  # fmt: skip
    if rc != 0:
        raise capi.MmxError(rc, capi.lib().mmx_last_error().decode())
    torch.cuda.synchronize()
    return dict(H=cpu(H), g=cpu(g), err=cpu(e))


def _same(a, b, keys=("H", "g", "err")):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def _check_symmetric(H):
    assert np.array_equal(H, np.swapaxes(H, 1, 2)), "H is not bitwise symmetric"


def _check_g_err(got, one):
    """g and err of a split call against the unsplit call on the same inputs (module docstring)."""
    for b in range(one["g"].shape[0]):
        dg, scale = np.abs(got["g"][b].astype(np.float64) - one["g"][b]).max(), np.abs(one["g"][b]).max()
        assert dg <= 2.0**-23 * scale, (b, dg, scale)
        assert abs(got["err"][b] - one["err"][b]) <= 2.0**-40 * one["err"][b], (b, got["err"][b], one["err"][b])


def _dist(x, x64):
    B = x64.shape[0]
    x, x64 = np.asarray(x, np.float64).reshape(B, -1), np.asarray(x64, np.float64).reshape(B, -1)
    scale = np.abs(x64).max(axis=1)
    return np.abs(x - x64).max(axis=1) / np.where(scale > 0, scale, 1.0)


def _compare(name, got, want64, want32, keys=("H", "g", "err")):
    fails = []
    for key in keys:
        d32, dg = _dist(want32[key], want64[key]).max(), _dist(got[key], want64[key]).max()
        bound = max(4 * d32, FLOOR)
        _parity[f"{name}/{key}"] = dict(gpu=float(dg), d32=float(d32), bound=float(bound))
        print(f"{name}/{key}: gpu {dg:.3e}  d32 {d32:.3e}  bound {bound:.3e}")
        assert np.isfinite(got[key]).all(), (name, key)
        if not dg <= bound:
            fails.append((key, dg, bound))
    assert not fails, (name, fails)


# name: (case, B, C, S, plane) -- the shapes of tests/test_gpu_vertex_normal_equations.py that this file reuses, with its seeds
SHAPES = dict(
    plane_c65=("character24", 2, 65, 1, True),
    position_c11=("character24", 2, 11, 1, False),  # 33 rows: the boundary at row 32 lies inside constraint 10
    position_c22=("character24", 2, 22, 1, False),  # 66 rows: the boundary at row 32 inside constraint 10, at 64 inside 21
    humanoid_triangles=("humanoid", 2, 200, 3, False),  # S = 3, 600 rows, T = 19, n = 128: all ten blocks
    k8=("k8", 2, 20, 3, True),  # (one tile: the effective parts is 1)
    k8_c100=("k8", 2, 100, 3, True),  # ... and the same skin with four tiles
    random_tree=("random_tree", 2, 25, 3, False),  # 75 rows, T = 3
)


def _shape(name):
    """(case name, theta, constraints, float64 reference, float32 reference) of a named shape, computed once."""
    if name not in _refs:
        cname, B, Cn, S, plane = SHAPES[name]
        case = _case(cname)
        theta = case.theta(B, 100 + len(name))
        con = _constraints(case.V, B, Cn, S, plane, 200 + len(name))
        _refs[name] = (cname, theta, con, case.reference(theta, con, torch.float64), case.reference(theta, con, torch.float32))
    return _refs[name]


# ---- 1
@pytest.mark.parametrize("name", ["plane_c65", "position_c22", "humanoid_triangles"])
def test_parts_one_is_the_unsplit_call(torch_cuda, name):
    cname, theta, con, _, _ = _shape(name)
    pb, skin = _problem(cname, 2), _case(cname).skin
    _same(_run(pb, skin, theta, con, parts=1, workspace=None), _run(pb, skin, theta, con))


# ---- 2
SLICED = [
    ("character24", True, 65, 1, (2, 3)),
    ("character24", True, 320, 1, (3, 4, 7, 10)),
    ("character24", False, 64, 1, (2,)),
    ("character24", False, 96, 1, (3,)),
    ("humanoid", False, 192, 3, (2, 3, 6)),
    ("random_tree", True, 96, 1, (3,)),
]


@pytest.mark.parametrize("cname,plane,Cn,S,parts_list", SLICED, ids=[f"{s[0]}_{'plane' if s[1] else 'position'}_c{s[2]}" for s in SLICED])
def test_split_is_the_fixed_order_sum_of_its_parts(torch_cuda, cname, plane, Cn, S, parts_list):
    case, B = _case(cname), 2
    pb = _problem(cname, B)
    theta = case.theta(B, 500 + Cn)
    con = _constraints(case.V, B, Cn, S, plane, 501 + Cn)
    T = _tiles(con)
    one = _run(pb, case.skin, theta, con)
    for parts in parts_list:
        assert parts <= T
        total = np.zeros(one["H"].shape, np.float64)
        for p in range(parts):
            t0, t1 = p * T // parts, (p + 1) * T // parts
            r0, r1 = 32 * t0, min(32 * t1, con.C if plane else 3 * con.C)
            assert plane or (r0 % 3 == 0 and r1 % 3 == 0), "the shape must put every part boundary on a constraint boundary"
            c0, c1 = (r0, r1) if plane else (r0 // 3, r1 // 3)
            total = total + _run(pb, case.skin, theta, _slice(con, c0, c1), want=("jtj",))["H"].astype(np.float64)
        got = _run(pb, case.skin, theta, con, parts=parts)
        assert np.array_equal(got["H"], total.astype(np.float32)), (parts, np.abs(got["H"] - total.astype(np.float32)).max())
        _check_symmetric(got["H"])
        _check_g_err(got, one)


# ---- 3
CUT = [("position_c22", 2), ("position_c22", 3), ("position_c11", 2), ("humanoid_triangles", 2), ("humanoid_triangles", 5),
       ("humanoid_triangles", 19), ("humanoid_triangles", 512), ("k8", 3), ("k8_c100", 3), ("random_tree", 3)]  # fmt: skip


@pytest.mark.parametrize("name,parts", CUT, ids=[f"{n}_p{p}" for n, p in CUT])
def test_parity_where_a_boundary_cuts_a_constraint(torch_cuda, name, parts):
    cname, theta, con, want64, want32 = _shape(name)
    pb, skin = _problem(cname, 2), _case(cname).skin
    got = _run(pb, skin, theta, con, parts=parts)
    _check_symmetric(got["H"])
    _compare(f"{name}/parts{parts}", got, want64, want32)
    _check_g_err(got, _run(pb, skin, theta, con))


def test_parity_instance_rest(torch_cuda):
    case, B = _case("character24"), 3
    theta = case.theta(B, 301)
    con = _constraints(case.V, B, 21, 3, False, 302)  # 63 rows, T = 2: the boundary at row 32 inside constraint 10
    rest = (case.arrays[3][None] + np.random.default_rng(303).normal(scale=0.05, size=(B, case.V, 3))).astype(np.float32)
    pb = _problem("character24", B)
    got = _run(pb, case.skin, theta, con, parts=3, rest=rest)
    _check_symmetric(got["H"])
    _compare("instance_rest/parts3", got, case.reference(theta, con, torch.float64, rest=rest), case.reference(theta, con, torch.float32, rest=rest))
    _check_g_err(got, _run(pb, case.skin, theta, con, rest=rest))
    assert not np.array_equal(_run(pb, case.skin, theta, con, parts=3)["g"], got["g"])


# ---- 4
def test_parts_beyond_the_tiles_is_parts_equal_tiles(torch_cuda):
    cname, theta, con, _, _ = _shape("plane_c65")
    assert _tiles(con) == 3
    pb, skin = _problem(cname, 2), _case(cname).skin
    three = _run(pb, skin, theta, con, parts=3)
    for parts in (4, 512):
        _same(_run(pb, skin, theta, con, parts=parts), three)
    assert not np.array_equal(three["H"], _run(pb, skin, theta, con, parts=2)["H"])  # (another association: other bits)


# ---- 5
def test_bits_depend_on_the_instance_and_the_effective_parts_only(torch_cuda):
    case = _case("humanoid")
    theta = case.theta(5, 361)
    con = _constraints(case.V, 5, 70, 3, False, 362)  # 210 rows, T = 7
    pb5 = _problem("humanoid", 5)
    first, second = _run(pb5, case.skin, theta, con, parts=3), _run(pb5, case.skin, theta, con, parts=3, fill=0x5A)
    _same(first, second)
    for b in (0, 3, 4):
        alone = _run(_problem("humanoid", 1), case.skin, theta[b : b + 1], _slice(con, 0, con.C, rows=slice(b, b + 1)), parts=3)
        for key in first:
            assert np.array_equal(first[key][b], alone[key][0]), (b, key)
    perm = np.array([3, 0, 4, 2, 1])
    moved = _run(pb5, case.skin, theta[perm], _slice(con, 0, con.C, rows=perm), parts=3)
    for key in first:
        assert np.array_equal(moved[key], first[key][perm]), key


# ---- 6
@pytest.mark.parametrize("n", [5, 33])
def test_parity_enabled_mask(torch_cuda, n):
    """n = 5: one block, three of the four waves hold none; n = 33: two block columns, three blocks."""
    case, B = _case("humanoid"), 2
    enabled = np.zeros(case.rig.num_params, bool)
    enabled[:3] = True  # the root translation moves every vertex
    enabled[3 + np.random.default_rng(320 + n).permutation(case.rig.num_params - 3)[: n - 3]] = True
    assert int(enabled.sum()) == n
    theta = case.theta(B, 321)
    con = _constraints(case.V, B, 40, 1, False, 322)  # 120 rows, T = 4
    pb = _problem("humanoid", B, enabled)
    got = _run(pb, case.skin, theta, con, parts=3)
    assert got["H"].shape == (B, n, n) and got["g"].shape == (B, n)
    _check_symmetric(got["H"])
    _compare(f"enabled_mask_n{n}/parts3", got, case.reference(theta, con, torch.float64, enabled=enabled), case.reference(theta, con, torch.float32, enabled=enabled))
    _check_g_err(got, _run(pb, case.skin, theta, con))


# ---- 7
def test_all_weights_zero_gives_exact_zeros(torch_cuda):
    case, B = _case("character24"), 2
    theta = case.theta(B, 331)
    for plane in (False, True):
        con = _constraints(case.V, B, 140, 3, plane, 332)  # 420 rows (T = 14) or 140 rows (T = 5)
        con.weight[:] = 0.0
        con.target[:] = np.nan  # behind zero weights: not read
        got = _run(_problem("character24", B), case.skin, theta, con, parts=4, fill=0xFF)
        assert not got["H"].any() and not got["g"].any() and not got["err"].any()
        assert not np.signbit(got["H"]).any() and not np.signbit(got["g"]).any()


def test_a_part_of_skipped_constraints_contributes_nothing(torch_cuda):
    """Part 1 of 3 (constraints 32..63 of 96 plane constraints) consists of skipped constraints only: zero, negative and NaN
    weights, -1 and out-of-range indices.  Their targets, normals and indices do not reach the result."""
    case, B = _case("character24"), 2
    theta = case.theta(B, 335)
    con = _constraints(case.V, B, 96, 1, True, 336)
    kinds = np.arange(32) % 5
    for b in range(B):
        w, v = con.weight[b, 32:64], con.vertex[b, 32:64, 0]
        w[kinds == 0], w[kinds == 1], w[kinds == 2] = 0.0, -2.0, np.nan
        v[kinds == 3] = -1
        v[kinds == 4] = np.array([case.V, case.V + 9, 2**31 - 1, 2**30, case.V, case.V + 1])[: (kinds == 4).sum()]
    assert not con.active(case.V)[:, 32:64].any() and con.active(case.V)[:, :32].all() and con.active(case.V)[:, 64:].all()
    pb = _problem("character24", B)
    got = _run(pb, case.skin, theta, con, parts=3)
    other = _slice(con, 0, con.C)
    other.target[:, 32:64] = np.nan
    other.normal[:, 32:64] = np.inf
    _same(_run(pb, case.skin, theta, other, parts=3), got)
    assert np.isfinite(got["H"]).all() and np.isfinite(got["g"]).all() and np.isfinite(got["err"]).all()
    # ... and it is the sum of the two other parts alone
    total = sum(_run(pb, case.skin, theta, _slice(con, c0, c1), want=("jtj",))["H"].astype(np.float64) for c0, c1 in ((0, 32), (64, 96)))
    assert np.array_equal(got["H"], total.astype(np.float32))


@pytest.mark.parametrize("S,plane", [(1, False), (3, True)])
def test_skipped_constraints(torch_cuda, S, plane):
    case, B, Cn = _case("character24"), 2, 45  # 135 rows (T = 5) or 45 rows (T = 2)
    theta = case.theta(B, 341)
    con = _constraints(case.V, B, Cn, S, plane, 342 + S)
    rng = np.random.default_rng(343)
    bad = rng.permutation(B * Cn)[:20].reshape(5, 4)
    at = lambda i: np.unravel_index(bad[i], (B, Cn))
    con.weight[at(0)], con.weight[at(1)], con.weight[at(2)] = 0.0, -1.5, np.nan
    con.vertex[at(3) + (np.arange(4) % S,)] = -1
    con.vertex[at(4) + ((np.arange(4) + 1) % S,)] = np.array([case.V, case.V + 7, 2**31 - 1, case.V])
    for i in range(3):
        con.target[at(i)] = np.nan
        if plane:
            con.normal[at(i)] = np.nan
        if S == 3:
            con.barycentric[at(i)] = np.inf
    assert con.active(case.V).sum() == B * Cn - 20
    pb = _problem("character24", B)
    got = _run(pb, case.skin, theta, con, parts=2)
    clean = con.without_skipped(case.V)
    _check_symmetric(got["H"])
    _compare(f"skipped_s{S}/parts2", got, case.reference(theta, clean, torch.float64), case.reference(theta, clean, torch.float32))
    _same(_run(pb, case.skin, theta, clean, parts=2), got)


# ---- 8
def test_nonfinite_target_stays_in_its_instance(torch_cuda):
    case, B = _case("character24"), 3
    theta = case.theta(B, 351)
    con = _constraints(case.V, B, 33, 1, False, 352)  # 99 rows, T = 4
    pb = _problem("character24", B)
    base = _run(pb, case.skin, theta, con, parts=3)
    con.target[1, 20, 2] = np.nan  # row 62: in the second of three parts; behind a positive weight: an ordinary input
    got = _run(pb, case.skin, theta, con, parts=3)
    assert np.isnan(got["err"][1]) and np.isnan(got["g"][1]).any()  # (H of position constraints does not read the targets)
    for b in (0, 2):
        for key in got:
            assert np.array_equal(got[key][b], base[key][b]), (b, key)
            assert np.isfinite(got[key][b]).all()


# ---- 9
def test_output_bits_do_not_depend_on_the_outputs_requested(torch_cuda):
    case, B = _case("humanoid"), 2
    theta = case.theta(B, 371)
    con = _constraints(case.V, B, 150, 3, True, 372)  # T = 5
    pb = _problem("humanoid", B)
    full = _run(pb, case.skin, theta, con, parts=3)
    names = dict(jtj="H", jtr="g", err="err")
    for want in (("jtj",), ("jtr",), ("err",), ("jtj", "err"), ("jtr", "err"), ("jtj", "jtr")):
        got = _run(pb, case.skin, theta, con, parts=3, want=want, fill=0xFF)
        for w, key in names.items():
            if w in want:
                assert np.array_equal(got[key], full[key]), (want, key)
            else:
                assert got[key] is None


# ---- 10
def test_workspace_is_written_before_it_is_read(torch_cuda):
    """A workspace of exactly the reported size, prefilled with 0xFF bytes (NaN patterns in float and double) or with zeros."""
    cname, theta, con, _, _ = _shape("humanoid_triangles")
    pb, skin = _problem(cname, 2), _case(cname).skin
    for parts in (2, 5, 19):
        ones, zeros = _run(pb, skin, theta, con, parts=parts, fill=0xFF), _run(pb, skin, theta, con, parts=parts, fill=0)
        _same(ones, zeros)
        assert np.isfinite(ones["H"]).all() and np.isfinite(ones["g"]).all() and np.isfinite(ones["err"]).all()
    # the size is for the parts asked for: 512 parts of 19 tiles run in a 512-part workspace, and give the bits of 19
    _same(_run(pb, skin, theta, con, parts=512, fill=0xFF), _run(pb, skin, theta, con, parts=19, fill=0))


# ---- 11
def test_refusals_leave_outputs_and_workspace_untouched(torch_cuda):
    L = capi.lib()
    case, B = _case("character24"), 2
    other = Case.synthetic(make_test_character(3), 5, 2, 9)
    pb = _problem("character24", B)
    n, Cn = pb.n, 70  # T = 3
    con = _constraints(case.V, B, Cn, 3, True, 431)
    dev = dict(theta=_cuda(case.theta(B, 432)), target=_cuda(con.target), vertex=_cuda(con.vertex, np.int32), bary=_cuda(con.barycentric),
               normal=_cuda(con.normal), weight=_cuda(con.weight))  # fmt: skip
    H = torch.full((B, n, n), 7.0, device="cuda")
    g = torch.full((B, n), 7.0, device="cuda")
    e = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    need = capi.skin_normal_equations_workspace_bytes(B, n, 2)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(pb_h=pb._h, skin_h=case.skin._h, type_=_abi.MMX_VC_PLANE, count=Cn, corners=3, fw=1.0, theta=dev["theta"], outs=(H, g, e), desc=True,
             parts=2, ws_ptr=ws.data_ptr(), ws_bytes=need, refused=True, **arr):  # fmt: skip
        a = {k: arr.get(k, dev[k]) for k in ("vertex", "bary", "target", "normal", "weight")}
        d = _abi.VertexConstraints(type_, count, corners, fw, ptr(a["vertex"]), ptr(a["bary"]), ptr(a["target"]), ptr(a["normal"]), ptr(a["weight"]), None)
        rc = L.mmx_skin_normal_equations_split(pb_h, skin_h, C.byref(d) if desc else None, ptr(theta), *(ptr(o) for o in outs), parts, ws_ptr, ws_bytes, None)
        torch.cuda.synchronize()
        if refused:
            assert (H == 7.0).all() and (g == 7.0).all() and (e == 7.0).all(), "a refused call wrote to an output"
            assert (ws == 0x5A).all(), "a refused call wrote to the workspace"
        return rc, L.mmx_last_error().decode()

    split = [
        (dict(parts=-1), "negative"), (dict(parts=513), "MMX_SKIN_NE_MAX_PARTS"), (dict(ws_ptr=None), "null"), (dict(ws_ptr=None, ws_bytes=0), "null"),
        (dict(ws_bytes=need - 1), "workspace_bytes"), (dict(ws_bytes=0), "workspace_bytes"), (dict(ws_ptr=ws.data_ptr() + 4), "16-byte"),
        (dict(ws_ptr=ws.data_ptr() + 8), "16-byte"), (dict(parts=512), "workspace_bytes"),  # (the size is for the parts asked for)
    ]  # fmt: skip
    unsplit = [
        (dict(skin_h=other.skin._h), "another rig"), (dict(skin_h=None), "skin"), (dict(desc=False), "descriptor"), (dict(theta=None), "theta"),
        (dict(outs=(None, None, None)), "all null"), (dict(target=None), "target"), (dict(count=0), "count"), (dict(count=-3), "count"),
        (dict(corners=2), "corners"), (dict(corners=0), "corners"), (dict(type_=2), "type"), (dict(type_=-1), "type"),
        (dict(normal=None), "normals"), (dict(fw=float("nan")), "function_weight"), (dict(fw=-0.5), "function_weight"),
        (dict(fw=float("inf")), "function_weight"), (dict(vertex=None), "vertex"), (dict(bary=None), "barycentric"),
        (dict(vertex=None, corners=1, count=case.V - 1), "vertex"),
    ]  # fmt: skip
    for kw, word in split + unsplit:
        rc, msg = call(**kw)
        assert rc == MMX_ERR_INVALID_ARGUMENT and msg.startswith("mmx_skin_normal_equations_split: ") and word in msg, (kw, rc, msg)
    for kw, word in unsplit:  # an unsplit refusal comes first, whatever is wrong with parts or the workspace
        for more in (dict(parts=-1), dict(parts=513), dict(ws_ptr=None), dict(ws_ptr=ws.data_ptr() + 4)):
            rc, msg = call(**kw, **more)
            assert rc == MMX_ERR_INVALID_ARGUMENT and word in msg, (kw, more, rc, msg)
    rc, msg = call(parts=513, ws_ptr=None)  # the range of parts before the workspace
    assert rc == MMX_ERR_INVALID_ARGUMENT and "MMX_SKIN_NE_MAX_PARTS" in msg
    rc, msg = call(refused=False)
    assert rc == 0, msg  # (the same call without a fault runs; the outputs are overwritten now)
    assert not (H == 7.0).any() and not (g == 7.0).any() and not (e == 7.0).any()
    assert (ws[need:] == 0x5A).all(), "the call wrote past the reported size"
    other.close()
    # more enabled parameters than the accumulators take: humanoid72 p219 -- the unsplit scope limit through the new entry
    big = Case.synthetic(make_humanoid72(variant="p219", unit=0.01), 30, 2, 433)
    pb_all = capi.Problem(big.rh, 1, [0], [])
    try:
        code, msg = 0, ""
        try:
            _run(pb_all, big.skin, big.theta(1, 434), _constraints(big.V, 1, 50, 1, False, 435), parts=2, workspace=ws)
        except capi.MmxError as err:
            code, msg = err.code, str(err)
        assert code == MMX_ERR_UNSUPPORTED and "128" in msg, (code, msg)
    finally:
        pb_all.close(), big.close()
    # tables beyond a workgroup's LDS: a root with 1023 children -- the unsplit refusal whose fact (the LDS size) the intake also
    # hands to the plan; it comes first, at parts 2 as at parts 0, and leaves outputs and workspace untouched
    wide = fk.make_rig([-1] + [0] * 1023, [(0, 3, 0, 1.0)], 1, seed=7)
    wcase = Case(wide, [[0]], [[1.0]], None, [[0.1, 0.2, 0.3]])
    pb_wide = capi.Problem(wcase.rh, 1, [0], [])
    try:
        Cw = 64  # 192 rows, six tiles: a split would be in effect
        wdev = [torch.zeros((1, Cw), dtype=torch.int32, device="cuda"), torch.zeros((1, Cw, 3), device="cuda"), torch.zeros((1, 1), device="cuda")]
        Hw = torch.full((1, pb_wide.n, pb_wide.n), 7.0, device="cuda")
        gw = torch.full((1, pb_wide.n), 7.0, device="cuda")
        ew = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
        ws.fill_(0x5A)
        assert 0 < capi.skin_normal_equations_workspace_bytes(1, pb_wide.n, 2) <= need
        d = _abi.VertexConstraints(_abi.MMX_VC_POSITION, Cw, 1, 1.0, wdev[0].data_ptr(), None, wdev[1].data_ptr(), None, None, None)
        for parts, ws_ptr in ((2, ws.data_ptr()), (0, ws.data_ptr()), (2, None), (513, ws.data_ptr())):
            rc = L.mmx_skin_normal_equations_split(pb_wide._h, wcase.skin._h, C.byref(d), wdev[2].data_ptr(), Hw.data_ptr(), gw.data_ptr(), ew.data_ptr(),
                                                   parts, ws_ptr, need, None)  # fmt: skip
            msg = L.mmx_last_error().decode()
            torch.cuda.synchronize()
            assert rc == MMX_ERR_UNSUPPORTED and msg.startswith("mmx_skin_normal_equations_split: ") and "LDS budget" in msg, (parts, rc, msg)
            assert (Hw == 7.0).all() and (gw == 7.0).all() and (ew == 7.0).all() and (ws == 0x5A).all(), parts
    finally:
        pb_wide.close(), wcase.close()


# ---- 12
def test_auto_parts(torch_cuda):
    case = _case("humanoid")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B, Cn, S, plane in ((1, 300, 1, False), (2, 260, 3, True), (5, 90, 1, False)):
        pb = _problem("humanoid", B)
        auto = pb.vertex_normal_equations_parts(case.skin, Cn, plane=plane, corners=S)
        plans = [capi.skin_normal_equations_plan(B, Cn, plane=plane, compute_units=cus, workgroups_per_cu=w) for w in (2, 1)]
        print(f"auto parts B={B} C={Cn}: {auto} (plan at two / one workgroups per CU: {plans}, {cus} CUs)")
        assert auto == plans[0] or (auto == plans[1] and S == 3)  # (two workgroups' LDS fit for S = 1 on this rig)
        theta = case.theta(B, 451)
        con = _constraints(case.V, B, Cn, S, plane, 452)
        _same(_run(pb, case.skin, theta, con, parts=0, workspace=torch.empty((capi.skin_normal_equations_workspace_bytes(B, pb.n, auto),), dtype=torch.uint8, device="cuda") if auto > 1 else None),
              _run(pb, case.skin, theta, con, parts=auto))  # fmt: skip
        H, g, e = pb.vertex_normal_equations(case.skin, _cuda(theta), _cuda(con.target), vertex=_cuda(con.vertex[..., 0] if S == 1 else con.vertex, np.int32),
                                             barycentric=_cuda(con.barycentric), normal=_cuda(con.normal), weight=_cuda(con.weight), function_weight=con.fw,
                                             parts="auto")  # fmt: skip
        _same(dict(H=H.cpu().numpy(), g=g.cpu().numpy(), err=e.cpu().numpy()), _run(pb, case.skin, theta, con, parts=auto))
    assert _problem("humanoid", 1).vertex_normal_equations_parts(case.skin, 300, plane=False) == 29  # 29 tiles, one per part


# ---- 13
def test_replays_from_a_captured_graph(torch_cuda):
    case, B = _case("humanoid"), 2
    con = _constraints(case.V, B, 90, 3, True, 421)  # T = 3
    thetas = [case.theta(B, s) for s in (422, 423)]
    pb = _problem("humanoid", B)
    eager = [_run(pb, case.skin, th, con, parts=3) for th in thetas]  # (also the warm-up)
    dev = dict(theta=_cuda(thetas[0]), target=_cuda(con.target), vertex=_cuda(con.vertex, np.int32), bary=_cuda(con.barycentric),
               normal=_cuda(con.normal), weight=_cuda(con.weight))  # fmt: skip
    H = torch.zeros((B, pb.n, pb.n), device="cuda")
    g = torch.zeros((B, pb.n), device="cuda")
    e = torch.zeros((B,), dtype=torch.float64, device="cuda")
    ws = torch.empty((capi.skin_normal_equations_workspace_bytes(B, pb.n, 3),), dtype=torch.uint8, device="cuda")
    d = _abi.VertexConstraints(_abi.MMX_VC_PLANE, con.C, 3, con.fw, dev["vertex"].data_ptr(), dev["bary"].data_ptr(), dev["target"].data_ptr(),
                               dev["normal"].data_ptr(), dev["weight"].data_ptr(), None)  # fmt: skip
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = capi.lib().mmx_skin_normal_equations_split(
                pb._h, case.skin._h, C.byref(d), dev["theta"].data_ptr(), H.data_ptr(), g.data_ptr(), e.data_ptr(), 3, ws.data_ptr(), ws.numel(),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))  # fmt: skip
            assert rc == 0, capi.lib().mmx_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for k in (0, 1):
        dev["theta"].copy_(_cuda(thetas[k]))
        for t in (H, g, e):
            t.zero_()
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for key, t in (("H", H), ("g", g), ("err", e)):
            assert np.array_equal(t.cpu().numpy(), eager[k][key]), (k, key)


# ---- 14
def test_host_form_matches_the_device_form(torch_cuda):
    L = capi.lib()
    case, B = _case("character24"), 2
    pb = _problem("character24", B)
    theta = case.theta(B, 441)
    con = _constraints(case.V, B, 135, 3, True, 442)  # T = 5
    hp = lambda a: a.ctypes.data
    vtx = np.ascontiguousarray(con.vertex, np.int32)
    d = _abi.VertexConstraints(_abi.MMX_VC_PLANE, con.C, 3, con.fw, hp(vtx), hp(con.barycentric), hp(con.target), hp(con.normal), hp(con.weight), None)
    for parts in (3, 1, 0):
        want = _run(pb, case.skin, theta, con, parts=parts if parts else pb.vertex_normal_equations_parts(case.skin, con.C, plane=True, corners=3))
        H, g, e = np.zeros((B, pb.n, pb.n), np.float32), np.zeros((B, pb.n), np.float32), np.zeros(B, np.float64)
        assert L.mmx_skin_normal_equations_split_host(pb._h, case.skin._h, C.byref(d), hp(theta), hp(H), hp(g), hp(e), parts) == 0, L.mmx_last_error()
        assert np.array_equal(H, want["H"]) and np.array_equal(g, want["g"]) and np.array_equal(e, want["err"]), parts
    assert L.mmx_skin_normal_equations_split_host(pb._h, case.skin._h, C.byref(d), None, hp(H), hp(g), hp(e), 3) == MMX_ERR_INVALID_ARGUMENT
    assert L.mmx_skin_normal_equations_split_host(pb._h, case.skin._h, C.byref(d), hp(theta), hp(H), hp(g), hp(e), 513) == MMX_ERR_INVALID_ARGUMENT


# ---- 15
def _gn_loop(eval_terms, theta0, lam, steps, dtype):
    """theta -= cholesky_solve(H + lam I, g), the solve in float64; theta kept in `dtype`.  Returns (theta, errors before each step)."""
    theta, errs = np.array(theta0, dtype), []
    for _ in range(steps):
        H, g, e = eval_terms(theta)
        errs.append(np.asarray(e, np.float64))
        A = np.asarray(H, np.float64) + lam * np.eye(H.shape[-1])
        theta = (theta.astype(np.float64) - np.linalg.solve(A, np.asarray(g, np.float64)[..., None])[..., 0]).astype(dtype)
    return theta, np.stack(errs)


def test_gauss_newton_fit_with_split_terms(torch_cuda):
    """Ten Gauss-Newton steps towards the posed vertices of a known theta* on every vertex of the humanoid (V = 300: 900 rows,
    T = 29), the recipe of the unsplit test: with parts = 4 (through geometry.vertex_normal_equations) and with parts = 1 the
    error decreases wherever the float64 loop's does and ends below 1e-6 of its start, and the final theta is within four times
    the float32 reference loop's distance from the float64 reference loop -- the bound of the unsplit test, for both."""
    case, B, lam, steps = _case("humanoid"), 1, 1e-3, 10
    star = case.theta(B, 401)
    start = (star + np.random.default_rng(402).normal(scale=0.05, size=star.shape)).astype(np.float32)
    rt, sk = fk.RigTensors(case.rig), skr.SkinTensors(*case.arrays, case.rig.num_joints)
    target = skr.skin_points(sk, fk.skeleton_state(rt, torch.as_tensor(star.astype(np.float64)))).numpy().astype(np.float32)
    con = vcr.Constraints(target, None, None, None, None, 1.0)  # vertex = NULL: constraint c is vertex c

    def ref_terms(dtype):
        def f(theta):
            r = case.reference(np.asarray(theta, np.float64), con, dtype)
            return r["H"], r["g"], r["err"]
        return f

    th64, e64 = _gn_loop(ref_terms(torch.float64), start, lam, steps, np.float64)
    th32, _ = _gn_loop(ref_terms(torch.float32), start, lam, steps, np.float32)
    d32 = np.abs(th32 - th64).max()
    pb = _problem("humanoid", B)
    tgt = _cuda(con.target)
    eye = torch.eye(pb.n, dtype=torch.float64, device="cuda")
    for parts in (1, 4):
        theta, errs = _cuda(start), []
        for _ in range(steps):
            H, g, e = geometry.vertex_normal_equations(pb, case.skin, theta, tgt, parts=parts)
            errs.append(e.cpu().numpy())
            delta = torch.cholesky_solve(g.double()[..., None], torch.linalg.cholesky(H.double() + lam * eye))[..., 0]
            theta = (theta.double() - delta).float().contiguous()
        eg, thg = np.stack(errs), theta.cpu().numpy()
        dg = np.abs(thg - th64).max()
        print(f"gn_fit parts {parts}: |theta - theta64| gpu {dg:.3e}  float32 loop {d32:.3e}  errors {eg[:, 0]}")
        _parity[f"gn_fit/parts{parts}/theta"] = dict(gpu=float(dg), d32=float(d32), bound=float(4 * d32))
        assert np.isfinite(eg).all() and np.isfinite(thg).all()
        down = e64[1:] < e64[:-1]
        assert down[:3].all() and (eg[1:] < eg[:-1])[down].all(), (e64[:, 0], eg[:, 0])
        assert eg[-1, 0] < 1e-6 * eg[0, 0]
        assert dg <= 4 * d32, (parts, dg, d32)
