"""mmx_skin_normal_equations on the GPU against the float64 reference (tests/vertex_constraints_reference.py, checked on its
own in tests/test_vertex_constraints_reference.py).

Distance: per instance max|X - X64| / max|X64| for H and g, |err - err64| / err64 for the error; X64 is the reference in
float64 on the same float32 inputs.  Bound: max(4 x the distance of the same reference code run in float32, 16 x 2^-24) -- the
floor covers shapes where the float32 restatement happens to be exact.  Nothing of the bound comes from the kernel's output.

Measured on an MI355X (largest distance over the instances: gpu | d32 | bound; profiles/skin_normal_equations_parity.json,
written through MMX_PARITY_OUT):
    character3_position     H 1.56e-07 | 2.66e-07 | 1.06e-06   g 1.16e-07 | 2.47e-07 | 9.90e-07   err 1.11e-07 | 2.72e-07 | 1.09e-06
    plane_c31               H 2.77e-07 | 4.05e-07 | 1.62e-06   g 1.55e-07 | 9.15e-07 | 3.66e-06   err 8.35e-08 | 4.59e-07 | 1.84e-06
    plane_c32               H 3.05e-07 | 4.77e-07 | 1.91e-06   g 1.44e-07 | 8.34e-07 | 3.34e-06   err 6.18e-08 | 4.91e-07 | 1.96e-06
    plane_c33               H 3.60e-07 | 4.91e-07 | 1.96e-06   g 1.83e-07 | 1.88e-06 | 7.54e-06   err 3.11e-08 | 5.09e-07 | 2.04e-06
    plane_c64               H 2.23e-07 | 3.83e-07 | 1.53e-06   g 1.75e-07 | 1.03e-06 | 4.13e-06   err 6.77e-08 | 3.96e-07 | 1.58e-06
    plane_c65               H 2.26e-07 | 3.84e-07 | 1.54e-06   g 1.59e-07 | 6.87e-07 | 2.75e-06   err 1.03e-07 | 6.28e-07 | 2.51e-06
    position_c10            H 2.88e-07 | 3.52e-07 | 1.41e-06   g 1.27e-07 | 5.58e-07 | 2.23e-06   err 5.92e-08 | 6.27e-07 | 2.51e-06
    position_c11            H 2.26e-07 | 3.99e-07 | 1.59e-06   g 1.21e-07 | 6.52e-07 | 2.61e-06   err 8.41e-08 | 6.47e-07 | 2.59e-06
    position_c22            H 2.38e-07 | 2.57e-07 | 1.03e-06   g 1.06e-07 | 5.08e-07 | 2.03e-06   err 7.02e-09 | 5.24e-07 | 2.10e-06
    humanoid_triangles      H 2.86e-07 | 2.15e-07 | 9.54e-07   g 7.41e-08 | 2.53e-07 | 1.01e-06   err 4.35e-08 | 5.57e-08 | 9.54e-07
    humanoid_every_vertex   H 1.77e-07 | 9.88e-08 | 9.54e-07   g 2.56e-07 | 1.82e-07 | 9.54e-07   err 1.04e-07 | 9.36e-08 | 9.54e-07
    k1                      H 4.44e-07 | 4.30e-07 | 1.72e-06   g 1.69e-07 | 7.21e-07 | 2.89e-06   err 4.59e-08 | 6.44e-07 | 2.57e-06
    k8                      H 2.39e-07 | 7.69e-07 | 3.08e-06   g 2.09e-07 | 4.14e-07 | 1.65e-06   err 1.73e-07 | 1.13e-07 | 9.54e-07
    random_tree             H 4.32e-07 | 4.32e-07 | 1.73e-06   g 2.04e-07 | 2.07e-07 | 9.54e-07   err 9.22e-08 | 8.85e-08 | 9.54e-07
    random_tree_plane       H 5.37e-07 | 1.79e-07 | 9.54e-07   g 1.42e-07 | 3.30e-07 | 1.32e-06   err 1.21e-07 | 1.93e-07 | 9.54e-07
    instance_rest           H 3.35e-07 | 6.98e-07 | 2.79e-06   g 1.09e-07 | 3.89e-07 | 1.55e-06   err 9.81e-08 | 6.66e-08 | 9.54e-07
    instance_rig            H 9.04e-07 | 8.31e-07 | 3.33e-06   g 9.46e-07 | 1.91e-06 | 7.63e-06   err 8.96e-07 | 1.53e-06 | 6.10e-06
    enabled_mask            H 1.46e-07 | 9.65e-08 | 9.54e-07   g 1.31e-07 | 2.14e-07 | 9.54e-07   err 2.12e-08 | 1.51e-07 | 9.54e-07
    skipped_s1              H 5.29e-07 | 3.21e-07 | 1.29e-06   g 8.93e-08 | 2.55e-07 | 1.02e-06   err 9.61e-08 | 1.09e-07 | 9.54e-07
    skipped_s3              H 2.88e-07 | 3.82e-07 | 1.53e-06   g 1.40e-07 | 2.49e-07 | 9.97e-07   err 6.97e-08 | 8.99e-08 | 9.54e-07
    autograd_chain_s1       g 3.09e-07 | 1.42e-07 | 9.54e-07   err 1.02e-07 | 1.14e-07 | 9.54e-07
    autograd_kernel_s1      g 1.35e-07 | 1.42e-07 | 9.54e-07   err 5.12e-08 | 1.14e-07 | 9.54e-07
    autograd_chain_s3       g 2.93e-07 | 1.75e-07 | 9.54e-07   err 1.68e-07 | 1.46e-07 | 9.54e-07
    autograd_kernel_s3      g 9.93e-08 | 1.75e-07 | 9.54e-07   err 8.54e-08 | 1.46e-07 | 9.54e-07
    rigid_skin/vertex       H 1.75e-07 | 1.48e-07 | 9.54e-07   g 1.94e-07 | 5.48e-07 | 2.19e-06   err 2.80e-08 | 3.14e-07 | 1.26e-06
    rigid_skin/joint_block  H 1.09e-07 | 1.48e-07 | 9.54e-07   g 3.06e-07 | 5.48e-07 | 2.19e-06   err 2.10e-08 | 3.14e-07 | 1.26e-06
    gn_fit                  theta 1.26e-05 | 1.73e-05 | 6.94e-05
Every figure is inside its bound (the largest share of a bound: 0.56).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import _abi
from momentum_amd import autograd as mauto
from momentum_amd import capi, geometry, make_humanoid72, make_test_character, make_test_skin, make_test_skinned_mesh
from tests import skeleton_state_reference as fk
from tests import skinning_reference as skr
from tests import vertex_constraints_reference as vcr

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT, MMX_ERR_UNSUPPORTED = 1, 4
FLOOR = 16 * 2.0**-24
_parity = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    """MMX_PARITY_OUT=<file>: the measured distances of this run as JSON (how profiles/skin_normal_equations_parity.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _parity:
        unit = "per instance max|X - X_ref64| / max|X_ref64| (err: relative), largest over the instances; bound = max(4 x d32, 16 x 2^-24)"
        with open(out, "w") as f:
            json.dump(dict(unit=unit, shapes=_parity), f, indent=1)


def _cuda(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


class Case:
    """A rig, a skin on it (arrays and device handle) and problems on the rig by batch size."""

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

    def problem(self, B, enabled=None):
        pb = capi.Problem(self.rh, B, [0], [])  # (the position constraint on the root is never given data: it is not read)
        if enabled is not None:
            pb.set_enabled(enabled)
        return pb

    def theta(self, B, seed):
        return fk.random_inputs(self.rig, B, seed)[0]

    def close(self):
        """The skin before its rig: mmx_skin_destroy reads the rig the skin was created on."""
        self.skin.close()
        self.rh.close()

    def reference(self, theta, con, dtype, **kw):
        return vcr.normal_equations(self.rig, self.arrays, theta, con, dtype=dtype, **kw)


def _constraints(V, B, C, S, plane, seed, vertex_null=False, fw=0.7):
    rng = np.random.default_rng(seed)
    vertex = None if vertex_null else rng.integers(0, V, size=(B, C, S)).astype(np.int32)
    bary = rng.dirichlet(np.ones(3), size=(B, C)).astype(np.float32) if S == 3 else None
    normal = rng.normal(size=(B, C, 3)).astype(np.float32) if plane else None
    target = rng.normal(scale=0.5, size=(B, C, 3)).astype(np.float32)
    return vcr.Constraints(target, vertex, bary, normal, rng.uniform(0.5, 2.0, size=(B, C)).astype(np.float32), fw)


def _run_gpu(pb, skin, theta, con, rest=None, want=("jtj", "jtr", "err")):
    vertex = None if con.vertex is None else _cuda(con.vertex[..., 0] if con.S == 1 else con.vertex, np.int32)
    H, g, e = pb.vertex_normal_equations(
        skin, _cuda(theta), _cuda(con.target), vertex=vertex, barycentric=_cuda(con.barycentric), normal=_cuda(con.normal),
        weight=_cuda(con.weight), rest=_cuda(rest), function_weight=con.fw, want=want,
    )  # fmt: skip
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return dict(H=cpu(H), g=cpu(g), err=cpu(e))


def _refusal(pb, skin, theta, con):
    """(status, message) of a call that is expected to be refused.  The exception is not kept: its traceback would tie the
    handles in the frames below into a reference cycle, and the collector finalises a cycle's objects in no particular order
    -- a rig before the skin or the problem that was created on it."""
    try:
        _run_gpu(pb, skin, theta, con)
    except capi.MmxError as e:
        return e.code, str(e)
    return 0, ""


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


def _check_symmetric(H):
    assert np.array_equal(H, np.swapaxes(H, 1, 2)), "H is not bitwise symmetric"


def _character3():
    joint, weight, rest = skr.hand_skin("character3_k4")
    rig = make_test_character(3)
    return Case(rig, joint, weight, make_test_skin(rig, 1, 1, 0).inverse_bind, rest)


def _character24(V=80, K=2, seed=61, random_affine=True):
    return Case.synthetic(make_test_character(24), V, K, seed, random_affine)


def _humanoid():
    return Case.synthetic(make_humanoid72(variant="p128", unit=0.01), 300, 4, 42)


def _random_tree():
    rig = fk.all_dofs_rig(fk.random_tree(9, 3), seed=4)  # every dof of every joint: P = 63, scales included
    rig.pt_offsets = np.random.default_rng(5).uniform(-0.2, 0.2, size=7 * rig.num_joints).astype(np.float32)
    return Case.synthetic(rig, 40, 3, 6, True)


_cases = {}


def _case(name):
    """One handle set per rig for the module (the cases are read-only)."""
    if name not in _cases:
        _cases[name] = dict(character3=_character3, character24=_character24, humanoid=_humanoid, random_tree=_random_tree,
                            k1=lambda: _character24(60, 1, 62), k8=lambda: _character24(60, 8, 63))[name]()  # fmt: skip
    return _cases[name]


# name: (case, B, C, S, plane, vertex_null)
SHAPES = {"character3_position": ("character3", 3, 5, 1, False, False)}
for _c in (31, 32, 33, 64, 65):  # the 32-row tile: its last row, the first row of the next, two tiles and one more
    SHAPES[f"plane_c{_c}"] = ("character24", 2, _c, 1, True, False)
for _c in (10, 11, 22):  # 30, 33, 66 rows: a tile boundary inside a constraint (rows 30 31 | 32)
    SHAPES[f"position_c{_c}"] = ("character24", 2, _c, 1, False, False)
SHAPES.update(
    humanoid_triangles=("humanoid", 2, 200, 3, False, False),  # S = 3, random barycentrics, 600 rows, n = 128: all ten blocks
    humanoid_every_vertex=("humanoid", 2, 300, 1, True, True),  # vertex = NULL: constraint c is vertex c
    k1=("k1", 2, 20, 3, False, False),
    k8=("k8", 2, 20, 3, True, False),
    random_tree=("random_tree", 2, 25, 3, False, False),
    random_tree_plane=("random_tree", 2, 40, 1, True, False),
)


@pytest.mark.parametrize("name", list(SHAPES))
def test_parity(torch_cuda, name):
    cname, B, Cn, S, plane, vnull = SHAPES[name]
    case = _case(cname)
    theta = case.theta(B, 100 + len(name))
    con = _constraints(case.V, B, Cn, S, plane, 200 + len(name), vertex_null=vnull)
    got = _run_gpu(case.problem(B), case.skin, theta, con)
    _check_symmetric(got["H"])
    _compare(name, got, case.reference(theta, con, torch.float64), case.reference(theta, con, torch.float32))


def test_parity_instance_rest(torch_cuda):
    case, B = _case("character24"), 3
    theta = case.theta(B, 301)
    con = _constraints(case.V, B, 21, 3, False, 302)
    rest = (case.arrays[3][None] + np.random.default_rng(303).normal(scale=0.05, size=(B, case.V, 3))).astype(np.float32)
    got = _run_gpu(case.problem(B), case.skin, theta, con, rest=rest)
    _check_symmetric(got["H"])
    _compare("instance_rest", got, case.reference(theta, con, torch.float64, rest=rest), case.reference(theta, con, torch.float32, rest=rest))
    shared = _run_gpu(case.problem(B), case.skin, theta, con)
    assert not np.array_equal(shared["g"], got["g"])


def test_parity_instance_rig(torch_cuda):
    case, B = _case("character24"), 3
    rng = np.random.default_rng(311)
    J = case.rig.num_joints
    offset = (case.rig.translation_offset[None] + rng.normal(scale=0.1, size=(B, J, 3))).astype(np.float32)
    pre = rng.normal(size=(B, J, 4))
    pre = (pre / np.linalg.norm(pre, axis=-1, keepdims=True)).astype(np.float32)
    theta = case.theta(B, 312)
    con = _constraints(case.V, B, 33, 1, True, 313)
    pb = case.problem(B)
    pb.set_instance_rig(offset, pre)
    got = _run_gpu(pb, case.skin, theta, con)
    kw = dict(offset=offset, pre=pre)
    _compare("instance_rig", got, case.reference(theta, con, torch.float64, **kw), case.reference(theta, con, torch.float32, **kw))


def test_parity_enabled_mask(torch_cuda):
    """A third of the parameters off: the compaction of mmx_eval_normal_equations (enabled parameters, ascending); enabled
    parameters that move no constrained vertex get exact zeros."""
    case, B = _case("humanoid"), 2
    enabled = np.ones(case.rig.num_params, bool)
    enabled[1::3] = False
    theta = case.theta(B, 321)
    con = _constraints(case.V, B, 12, 1, False, 322)  # twelve vertices: most finger parameters move none of them
    got = _run_gpu(case.problem(B, enabled), case.skin, theta, con)
    want64 = case.reference(theta, con, torch.float64, enabled=enabled)
    n = int(enabled.sum())
    assert got["H"].shape == (B, n, n) and got["g"].shape == (B, n)
    _check_symmetric(got["H"])
    _compare("enabled_mask", got, want64, case.reference(theta, con, torch.float32, enabled=enabled))
    zero = ~np.abs(want64["J"]).any(axis=1)  # [B, n] structurally zero columns
    assert zero.any() and not zero.all()
    for b in range(B):
        assert not got["H"][b][zero[b]].any() and not got["H"][b][:, zero[b]].any() and not got["g"][b][zero[b]].any()


def test_all_weights_zero_gives_exact_zeros(torch_cuda):
    case, B = _case("character24"), 2
    theta = case.theta(B, 331)
    for plane in (False, True):
        con = _constraints(case.V, B, 40, 3, plane, 332)
        con.weight[:] = 0.0
        con.target[:] = np.nan  # behind zero weights: not read
        got = _run_gpu(case.problem(B), case.skin, theta, con)
        assert not got["H"].any() and not got["g"].any() and not got["err"].any()
        assert not np.signbit(got["H"]).any() and not np.signbit(got["g"]).any()


@pytest.mark.parametrize("S,plane", [(1, False), (3, True)])
def test_skipped_constraints(torch_cuda, S, plane):
    """Weights 0 / negative / NaN, index -1 and index >= V mixed in: the result meets the reference computed without them and
    stays finite with NaN targets (and normals, barycentrics) behind them."""
    case, B, Cn = _case("character24"), 2, 45
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
    got = _run_gpu(case.problem(B), case.skin, theta, con)
    clean = con.without_skipped(case.V)
    _check_symmetric(got["H"])
    _compare(f"skipped_s{S}", got, case.reference(theta, clean, torch.float64), case.reference(theta, clean, torch.float32))
    # ... and bit for bit what the call gives with the skipped constraints replaced by harmless zero-weight ones
    again = _run_gpu(case.problem(B), case.skin, theta, clean)
    for key in got:
        assert np.array_equal(got[key], again[key]), key


def test_nonfinite_target_stays_in_its_instance(torch_cuda):
    case, B = _case("character24"), 3
    theta = case.theta(B, 351)
    con = _constraints(case.V, B, 33, 1, False, 352)
    base = _run_gpu(case.problem(B), case.skin, theta, con)
    con.target[1, 4, 2] = np.nan  # behind a positive weight: an ordinary input
    got = _run_gpu(case.problem(B), case.skin, theta, con)
    assert np.isnan(got["err"][1]) and np.isnan(got["g"][1]).any()
    for b in (0, 2):
        for key in got:
            assert np.array_equal(got[key][b], base[key][b]), (b, key)


def test_instance_bits_do_not_depend_on_the_batch_or_the_run(torch_cuda):
    case = _case("humanoid")
    theta = case.theta(5, 361)
    con = _constraints(case.V, 5, 70, 3, False, 362)
    pb5 = case.problem(5)
    first, second = _run_gpu(pb5, case.skin, theta, con), _run_gpu(pb5, case.skin, theta, con)
    one = vcr.Constraints(con.target[3:4], con.vertex[3:4], con.barycentric[3:4], None, con.weight[3:4], con.fw)
    alone = _run_gpu(case.problem(1), case.skin, theta[3:4], one)
    for key in first:
        assert np.array_equal(first[key], second[key]), key
        assert np.array_equal(first[key][3], alone[key][0]), key


def test_output_bits_do_not_depend_on_the_outputs_requested(torch_cuda):
    case, B = _case("humanoid"), 2
    theta = case.theta(B, 371)
    con = _constraints(case.V, B, 50, 3, True, 372)
    pb = case.problem(B)
    full = _run_gpu(pb, case.skin, theta, con)
    names = dict(jtj="H", jtr="g", err="err")
    for want in (("jtj",), ("jtr",), ("err",), ("jtj", "err"), ("jtr", "err"), ("jtj", "jtr")):
        got = _run_gpu(pb, case.skin, theta, con, want=want)
        for w, key in names.items():
            if w in want:
                assert np.array_equal(got[key], full[key]), (want, key)
            else:
                assert got[key] is None


def test_gradient_is_half_the_autograd_chain(torch_cuda):
    """g = J^T (sigma f) is half the theta-gradient of L = sum fw w |f|^2 through the existing differentiable stages
    (autograd.skeleton_state -> autograd.skin_points), which have their own oracles."""
    case, B = _case("humanoid"), 2
    theta = case.theta(B, 381)
    for S, plane in ((1, False), (3, True)):
        con = _constraints(case.V, B, 60, S, plane, 382 + S)
        pb = case.problem(B)
        got = _run_gpu(pb, case.skin, theta, con)
        th = _cuda(theta).requires_grad_(True)
        out = mauto.skin_points(case.skin, mauto.skeleton_state(pb, th))
        idx = torch.from_numpy(con.vertex.astype(np.int64)).cuda()
        corners = out[torch.arange(B, device="cuda")[:, None, None], idx]  # [B, C, S, 3]
        x = (_cuda(con.barycentric)[..., None] * corners).sum(2) if S == 3 else corners[:, :, 0]
        d = x - _cuda(con.target)
        f2 = ((_cuda(con.normal) * d).sum(-1)) ** 2 if plane else (d * d).sum(-1)
        L = (con.fw * _cuda(con.weight) * f2).sum()
        L.backward()
        chain = dict(g=0.5 * th.grad.cpu().numpy(), err=(con.fw * _cuda(con.weight) * f2).sum(1).detach().cpu().numpy())
        want64, want32 = case.reference(theta, con, torch.float64), case.reference(theta, con, torch.float32)
        _compare(f"autograd_chain_s{S}", chain, want64, want32, keys=("g", "err"))
        _compare(f"autograd_kernel_s{S}", got, want64, want32, keys=("g", "err"))
        assert _dist(got["g"], chain["g"]).max() <= 2 * max(4 * _dist(want32["g"], want64["g"]).max(), FLOOR)


def test_rigid_skin_is_the_position_block(torch_cuda):
    """A skin with K = 1, weight 1, identity inverse bind and rest = the constraint offset turns vertex position constraints
    into the position block of a problem on the same joints: H, g and err of Problem.normal_equations, in order and value.
    Pins the column order, the compaction and the sign of g."""
    rig = make_humanoid72(variant="p128", unit=0.01)
    B, Kp = 2, 17
    rng = np.random.default_rng(391)
    parents = rng.integers(0, rig.num_joints, size=Kp).astype(np.int32)
    offsets = rng.normal(scale=0.05, size=(Kp, 3)).astype(np.float32)
    case = Case(rig, parents[:, None], np.ones((Kp, 1), np.float32), None, offsets)
    enabled = np.ones(rig.num_params, bool)
    enabled[2::5] = False
    theta = case.theta(B, 392)
    target = rng.normal(scale=0.3, size=(B, Kp, 3)).astype(np.float32)
    weight = rng.uniform(0.5, 2.0, size=(B, Kp)).astype(np.float32)
    pb = capi.Problem(case.rh, B, list(parents), [])
    pb.set_enabled(enabled)
    pb.set_constraints(np.broadcast_to(offsets, (B, Kp, 3)), target, weight, np.zeros((B, 0, 4)), np.zeros((B, 0, 4)), np.zeros((B, 0)), pos_function_weight=0.7)
    Hj, gj, ej = pb.normal_equations(_cuda(theta))
    torch.cuda.synchronize()
    joints = dict(H=Hj.cpu().numpy(), g=gj.cpu().numpy(), err=ej.cpu().numpy())
    con = vcr.Constraints(target, None, None, None, weight, 0.7)
    got = _run_gpu(pb, case.skin, theta, con)  # vertex = NULL: C = V = Kp
    want64 = case.reference(theta, con, torch.float64, enabled=enabled)
    want32 = case.reference(theta, con, torch.float32, enabled=enabled)
    _compare("rigid_skin/vertex", got, want64, want32)
    _compare("rigid_skin/joint_block", joints, want64, want32)


def _gn_loop(eval_terms, theta0, lam, steps, dtype):
    """theta -= cholesky_solve(H + lam I, g), the solve in float64; theta kept in `dtype`.  Returns (theta, errors before each step)."""
    theta, errs = np.array(theta0, dtype), []
    for _ in range(steps):
        H, g, e = eval_terms(theta)
        errs.append(np.asarray(e, np.float64))
        A = np.asarray(H, np.float64) + lam * np.eye(H.shape[-1])
        theta = (theta.astype(np.float64) - np.linalg.solve(A, np.asarray(g, np.float64)[..., None])[..., 0]).astype(dtype)
    return theta, np.stack(errs)


def test_gauss_newton_fit_of_a_posed_mesh(torch_cuda):
    """Ten steps theta -= cholesky_solve(H + lambda I, g) towards the posed vertices of a known theta*, from theta* plus a
    perturbation: on the device with the kernel's terms (the solve in torch float64 on the device), on the CPU with the float64
    reference and with the float32 reference.  The error decreases wherever the float64 loop's does; the final theta is within
    four times the float32 loop's distance from the float64 loop."""
    case, B, lam, steps = _case("humanoid"), 1, 1e-3, 10
    star = case.theta(B, 401)
    start = (star + np.random.default_rng(402).normal(scale=0.05, size=star.shape)).astype(np.float32)
    rt, sk = fk.RigTensors(case.rig), skr.SkinTensors(*case.arrays, case.rig.num_joints)
    target = skr.skin_points(sk, fk.skeleton_state(rt, torch.as_tensor(star.astype(np.float64)))).numpy().astype(np.float32)
    con = vcr.Constraints(target, None, None, None, None, 1.0)

    def ref_terms(dtype):
        def f(theta):
            r = case.reference(np.asarray(theta, np.float64), con, dtype)
            return r["H"], r["g"], r["err"]
        return f

    th64, e64 = _gn_loop(ref_terms(torch.float64), start, lam, steps, np.float64)
    th32, e32 = _gn_loop(ref_terms(torch.float32), start, lam, steps, np.float32)
    pb = case.problem(B)
    theta, tgt = _cuda(start), _cuda(target)
    eye = torch.eye(pb.n, dtype=torch.float64, device="cuda")
    errs = []
    for _ in range(steps):
        H, g, e = pb.vertex_normal_equations(case.skin, theta, tgt)
        errs.append(e.cpu().numpy())
        delta = torch.cholesky_solve(g.double()[..., None], torch.linalg.cholesky(H.double() + lam * eye))[..., 0]
        theta = (theta.double() - delta).float().contiguous()
    eg, thg = np.stack(errs), theta.cpu().numpy()
    d32, dg = np.abs(th32 - th64).max(), np.abs(thg - th64).max()
    print(f"gn_fit: err64 {e64[:, 0]}\n        errgpu {eg[:, 0]}\n        |theta - theta64| gpu {dg:.3e}  float32 loop {d32:.3e}")
    _parity["gn_fit/theta"] = dict(gpu=float(dg), d32=float(d32), bound=float(4 * d32))
    assert np.isfinite(eg).all() and np.isfinite(thg).all()
    down = e64[1:] < e64[:-1]
    assert down[:3].all() and (eg[1:] < eg[:-1])[down].all(), (e64[:, 0], eg[:, 0])
    assert eg[-1, 0] < 1e-6 * eg[0, 0]
    assert dg <= 4 * d32, (dg, d32)


def test_point_to_plane_icp_with_closest_points_on_mesh(torch_cuda):
    """Correspondences from find_closest_points_on_mesh in every step (S = 3: faces[face_index] and the barycentrics as they
    come, -1 rows included), plane type with the posed mesh's vertex normals: the error decreases over the run."""
    rig = make_humanoid72(variant="p128", unit=0.01)
    s, tri = make_test_skinned_mesh(rig, 20, 15, 4, 411)
    case = Case(rig, s.joint, s.weight, s.inverse_bind, s.rest)
    mesh = capi.Mesh(tri, case.V)
    faces = torch.from_numpy(tri.astype(np.int64)).cuda()
    B, lam = 1, 1e-2
    star = case.theta(B, 412)
    start = (star + np.random.default_rng(413).normal(scale=0.02, size=star.shape)).astype(np.float32)
    pb = case.problem(B)
    scan = case.skin.skin_points(pb.skeleton_state(_cuda(star)))  # the points to fit: the mesh posed at theta*
    theta = _cuda(start)
    eye = torch.eye(pb.n, dtype=torch.float64, device="cuda")
    errs = []
    for _ in range(8):
        posed = case.skin.skin_points(pb.skeleton_state(theta))
        valid, _, face, bary = geometry.find_closest_points_on_mesh(scan, posed, mesh)
        corners = torch.where(face[..., None] >= 0, faces[face.clamp(min=0).long()], torch.full((), -1, device="cuda", dtype=torch.int64))
        vn = geometry.compute_vertex_normals(posed, mesh)
        normal = (bary[..., None] * vn[torch.arange(B, device="cuda")[:, None, None], corners.clamp(min=0)]).sum(2)
        H, g, e = geometry.vertex_normal_equations(pb, case.skin, theta, scan, vertex=corners, barycentric=bary, normal=normal, weight=valid)
        assert torch.isfinite(H).all() and torch.isfinite(g).all() and torch.isfinite(e).all()
        errs.append(float(e[0]))
        delta = torch.cholesky_solve(g.double()[..., None], torch.linalg.cholesky(H.double() + lam * eye))[..., 0]
        theta = (theta.double() - delta).float().contiguous()
    print("icp errors:", errs)
    assert errs[-1] < 0.5 * errs[0], errs


def test_replays_from_a_captured_graph(torch_cuda):
    case, B = _case("humanoid"), 2
    con = _constraints(case.V, B, 90, 3, True, 421)
    thetas = [case.theta(B, s) for s in (422, 423)]
    pb = case.problem(B)
    eager = [_run_gpu(pb, case.skin, th, con) for th in thetas]  # (also the warm-up)
    dev = dict(theta=_cuda(thetas[0]), target=_cuda(con.target), vertex=_cuda(con.vertex, np.int32), bary=_cuda(con.barycentric),
               normal=_cuda(con.normal), weight=_cuda(con.weight))  # fmt: skip
    H = torch.zeros((B, pb.n, pb.n), device="cuda")
    g = torch.zeros((B, pb.n), device="cuda")
    e = torch.zeros((B,), dtype=torch.float64, device="cuda")
    d = _abi.VertexConstraints(_abi.MMX_VC_PLANE, con.C, 3, con.fw, dev["vertex"].data_ptr(), dev["bary"].data_ptr(), dev["target"].data_ptr(),
                               dev["normal"].data_ptr(), dev["weight"].data_ptr(), None)  # fmt: skip
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = capi.lib().mmx_skin_normal_equations(pb._h, case.skin._h, C.byref(d), dev["theta"].data_ptr(), H.data_ptr(), g.data_ptr(), e.data_ptr(),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))  # fmt: skip
            assert rc == 0, capi.lib().mmx_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for k in (0, 1, 0):
        dev["theta"].copy_(_cuda(thetas[k]))
        for t in (H, g, e):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, t in (("H", H), ("g", g), ("err", e)):
            assert np.array_equal(t.cpu().numpy(), eager[k][key]), (k, key)


def test_refusals_leave_the_outputs_untouched(torch_cuda):
    L = capi.lib()
    case, B = _case("character24"), 2
    other = _character3()
    pb = case.problem(B)
    n, Cn = pb.n, 6
    con = _constraints(case.V, B, Cn, 3, True, 431)
    dev = dict(theta=_cuda(case.theta(B, 432)), target=_cuda(con.target), vertex=_cuda(con.vertex, np.int32), bary=_cuda(con.barycentric),
               normal=_cuda(con.normal), weight=_cuda(con.weight))  # fmt: skip
    H = torch.full((B, n, n), 7.0, device="cuda")
    g = torch.full((B, n), 7.0, device="cuda")
    e = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(pb_h=pb._h, skin_h=case.skin._h, type_=_abi.MMX_VC_PLANE, count=Cn, corners=3, fw=1.0, theta=dev["theta"], outs=(H, g, e), desc=True, refused=True, **arr):
        a = {k: arr.get(k, dev[k]) for k in ("vertex", "bary", "target", "normal", "weight")}
        d = _abi.VertexConstraints(type_, count, corners, fw, ptr(a["vertex"]), ptr(a["bary"]), ptr(a["target"]), ptr(a["normal"]), ptr(a["weight"]), None)
        rc = L.mmx_skin_normal_equations(pb_h, skin_h, C.byref(d) if desc else None, ptr(theta), *(ptr(o) for o in outs), None)
        torch.cuda.synchronize()
        assert not refused or ((H == 7.0).all() and (g == 7.0).all() and (e == 7.0).all()), "a refused call wrote to an output"
        return rc, L.mmx_last_error().decode()

    invalid = [
        (dict(skin_h=other.skin._h), "another rig"), (dict(skin_h=None), "skin"), (dict(desc=False), "descriptor"), (dict(theta=None), "theta"),
        (dict(outs=(None, None, None)), "all null"), (dict(target=None), "target"), (dict(count=0), "count"), (dict(count=-3), "count"),
        (dict(corners=2), "corners"), (dict(corners=0), "corners"), (dict(type_=2), "type"), (dict(type_=-1), "type"),
        (dict(normal=None), "normals"), (dict(fw=float("nan")), "function_weight"), (dict(fw=-0.5), "function_weight"),
        (dict(fw=float("inf")), "function_weight"), (dict(vertex=None), "vertex"), (dict(bary=None), "barycentric"),
        (dict(vertex=None, corners=1, count=case.V - 1), "vertex"),
    ]  # fmt: skip
    for kw, word in invalid:
        rc, msg = call(**kw)
        assert rc == MMX_ERR_INVALID_ARGUMENT and "mmx_skin_normal_equations" in msg and word in msg, (kw, rc, msg)
    rc, msg = call(refused=False)
    assert rc == 0, msg  # (the same call without a fault runs; the outputs are overwritten now)
    assert not (H == 7.0).any() and not (g == 7.0).any() and not (e == 7.0).any()
    other.close()
    # more enabled parameters than the accumulators take: humanoid72 p219
    big = Case.synthetic(make_humanoid72(variant="p219", unit=0.01), 30, 2, 433)
    enabled = np.zeros(big.rig.num_params, bool)
    enabled[:128] = True
    pb_all, pb_128 = big.problem(1), big.problem(1, enabled)
    try:
        code, msg = _refusal(pb_all, big.skin, big.theta(1, 434), _constraints(big.V, 1, 5, 1, False, 435))
        assert code == MMX_ERR_UNSUPPORTED and "128" in msg, (code, msg)
        ok = _run_gpu(pb_128, big.skin, big.theta(1, 434), _constraints(big.V, 1, 5, 1, False, 435))
        assert ok["H"].shape == (1, 128, 128) and np.isfinite(ok["H"]).all()
    finally:
        pb_all.close(), pb_128.close(), big.close()
    # tables beyond a workgroup's LDS: a root with 1023 children (the forward kinematics' buffers of 1024 joints exceed 160 KB)
    wide = fk.make_rig([-1] + [0] * 1023, [(0, 3, 0, 1.0)], 1, seed=7)
    wcase = Case(wide, [[0]], [[1.0]], None, [[0.1, 0.2, 0.3]])
    pb_wide = wcase.problem(1)
    try:
        code, msg = _refusal(pb_wide, wcase.skin, np.zeros((1, 1), np.float32), vcr.Constraints(np.zeros((1, 1, 3), np.float32)))
        assert code == MMX_ERR_UNSUPPORTED and "LDS budget" in msg, (code, msg)
    finally:
        pb_wide.close(), wcase.close()


def test_host_form_matches_the_device_form(torch_cuda):
    L = capi.lib()
    case, B = _case("character24"), 2
    pb = case.problem(B)
    theta = case.theta(B, 441)
    con = _constraints(case.V, B, 35, 3, True, 442)
    want = _run_gpu(pb, case.skin, theta, con)
    hp = lambda a: a.ctypes.data
    vtx = np.ascontiguousarray(con.vertex, np.int32)
    d = _abi.VertexConstraints(_abi.MMX_VC_PLANE, con.C, 3, con.fw, hp(vtx), hp(con.barycentric), hp(con.target), hp(con.normal), hp(con.weight), None)
    H, g, e = np.zeros((B, pb.n, pb.n), np.float32), np.zeros((B, pb.n), np.float32), np.zeros(B, np.float64)
    assert L.mmx_skin_normal_equations_host(pb._h, case.skin._h, C.byref(d), hp(theta), hp(H), hp(g), hp(e)) == 0, L.mmx_last_error()
    assert np.array_equal(H, want["H"]) and np.array_equal(g, want["g"]) and np.array_equal(e, want["err"])
    assert L.mmx_skin_normal_equations_host(pb._h, case.skin._h, C.byref(d), None, hp(H), hp(g), hp(e)) == MMX_ERR_INVALID_ARGUMENT
