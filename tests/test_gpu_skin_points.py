"""mmx_skin_points / mmx_skin_points_backward on the GPU against the float64 reference and its autograd gradients
(tests/skinning_reference.py, checked on its own in tests/test_skinning_reference.py).

Distance: max|x_gpu - x_ref64| / max|x_ref64| per instance, for out, state_grad and rest_grad alike.  Yardstick: the same
reference run in float32 on the CPU, whose distance d32 from the float64 run is computed here for the same inputs; the GPU must
stay within 4 x the largest d32 over the test's instances (the factor covers the different summation order: per joint, lanes
stride the joint-sorted influence list and a cross-lane tree follows, where torch scatters vertex by vertex).  States come
from Problem.skeleton_state at random theta (rotations +-1 rad, translations +-0.2, scales +-0.3) and are handed to the GPU
and to the reference alike, so only skinning is compared; cotangents are standard-normal; fixed seeds.

Measured on an MI355X (largest distance over the instances, gpu | d32 | bound = 4 x d32; profiles/skin_points_parity.json,
written through MMX_PARITY_OUT):
    one_joint                      out 5.32e-08 | 6.17e-08 | 2.47e-07   state_grad 3.38e-08 | 7.41e-08 | 2.97e-07   rest_grad 6.47e-08 | 7.68e-08 | 3.07e-07
    character3_k4_b1               out 7.67e-08 | 1.05e-07 | 4.21e-07   state_grad 2.84e-08 | 4.03e-08 | 1.61e-07   rest_grad 5.06e-08 | 3.56e-08 | 1.43e-07
    character3_k4_b5               out 7.67e-08 | 1.05e-07 | 4.21e-07   state_grad 2.84e-08 | 1.20e-07 | 4.81e-07   rest_grad 8.39e-08 | 7.31e-08 | 2.92e-07
    one_joint_heavy                out 1.19e-07 | 1.38e-07 | 5.50e-07   state_grad 2.38e-08 | 4.23e-07 | 1.69e-06   rest_grad 7.69e-08 | 1.31e-07 | 5.24e-07
    k8                             out 1.51e-07 | 1.21e-07 | 4.85e-07   state_grad 3.35e-08 | 4.28e-07 | 1.71e-06   rest_grad 9.75e-08 | 1.24e-07 | 4.98e-07
    humanoid72                     out 1.49e-07 | 1.36e-07 | 5.44e-07   state_grad 5.01e-08 | 5.56e-07 | 2.22e-06   rest_grad 9.18e-08 | 1.37e-07 | 5.47e-07
    rig300                         out 1.61e-07 | 1.52e-07 | 6.07e-07   state_grad 4.61e-08 | 1.80e-07 | 7.22e-07   rest_grad 1.02e-07 | 1.50e-07 | 6.01e-07
    edge_v1023                     out 1.23e-07 | 8.98e-08 | 3.59e-07   state_grad 3.83e-08 | 1.09e-06 | 4.36e-06   rest_grad 7.24e-08 | 1.06e-07 | 4.25e-07
    edge_v1024                     out 1.32e-07 | 9.09e-08 | 3.64e-07   state_grad 2.57e-08 | 8.80e-07 | 3.52e-06   rest_grad 8.04e-08 | 9.03e-08 | 3.61e-07
    edge_v1025                     out 1.25e-07 | 9.72e-08 | 3.89e-07   state_grad 3.19e-08 | 1.08e-06 | 4.32e-06   rest_grad 7.98e-08 | 9.65e-08 | 3.86e-07
    edge_v63                       out 9.44e-08 | 9.44e-08 | 3.78e-07   state_grad 4.40e-08 | 3.85e-07 | 1.54e-06   rest_grad 8.71e-08 | 1.05e-07 | 4.19e-07
    edge_v64                       out 7.86e-08 | 7.86e-08 | 3.14e-07   state_grad 3.75e-08 | 1.91e-07 | 7.66e-07   rest_grad 8.66e-08 | 8.69e-08 | 3.48e-07
    edge_v65                       out 1.12e-07 | 7.44e-08 | 2.97e-07   state_grad 4.85e-08 | 4.46e-07 | 1.78e-06   rest_grad 6.42e-08 | 8.58e-08 | 3.43e-07
    one_hot_character3             out 2.82e-08 | 2.82e-08 | 1.13e-07   state_grad 4.76e-08 | 1.25e-07 | 5.01e-07   rest_grad 5.24e-08 | 7.18e-08 | 2.87e-07
    character3_k4_b5_instance_rest out 2.12e-07 | 9.98e-08 | 3.99e-07   state_grad 3.34e-08 | 1.62e-07 | 6.49e-07   rest_grad 1.06e-07 | 9.88e-08 | 3.95e-07
    k8_instance_rest               out 1.73e-07 | 1.68e-07 | 6.73e-07   state_grad 4.24e-08 | 6.71e-07 | 2.68e-06   rest_grad 8.63e-08 | 8.63e-08 | 3.45e-07
    end_to_end_chain24             vertices 4.90e-07 | 3.24e-07 | 1.29e-06   theta_grad 3.26e-07 | 2.47e-07 | 9.86e-07
    end_to_end_humanoid72          vertices 4.44e-07 | 6.37e-07 | 2.55e-06   theta_grad 2.53e-07 | 3.06e-07 | 1.22e-06
Every figure is inside its bound.  The kernels build each joint's posed affine in double and round it once, and take the
backward sums in double: the state gradient sits at 2e-8 to 5e-8 where the float32 reference's scatter is at 4e-8 to 1.1e-6.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import _abi
from momentum_amd import autograd as mauto
from momentum_amd import capi, make_humanoid72, make_rig300, make_test_character, make_test_skin
from tests import skeleton_state_reference as fk
from tests import skinning_reference as ref

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT, MMX_ERR_UNSUPPORTED = 1, 4
TILE = 1024  # kSkinTile: vertices of one instance a forward workgroup takes (momentum_amd/csrc/mmx_kernels.hpp)
_parity = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    """MMX_PARITY_OUT=<file>: the measured distances of this run as JSON (how profiles/skin_points_parity.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _parity:
        with open(out, "w") as f:
            json.dump(dict(unit="max|x - x_ref64| / max|x_ref64| per instance, largest over the instances; bound = 4 x d32", shapes=_parity), f, indent=1)


class Case:
    """A rig, a skin on it (arrays, device handle, reference tensors) and the rig's problem handle for the states."""

    def __init__(self, rig, joint, weight, inverse_bind, rest):
        self.rig, self.J = rig, rig.num_joints
        self.joint, self.weight = np.asarray(joint, np.int32), np.asarray(weight, np.float32)
        self.inv, self.rest = inverse_bind, np.asarray(rest, np.float32)
        self.rh = capi.RigHandle(rig, 0)
        self.skin = capi.Skin(self.rh, self.joint, self.weight, self.inv, self.rest)
        self.V, self.K = self.joint.shape

    @classmethod
    def synthetic(cls, rig, V, K, seed, random_affine=False):
        s = make_test_skin(rig, V, K, seed, random_affine)
        return cls(rig, s.joint, s.weight, s.inverse_bind, s.rest)

    def tensors(self, dtype):
        return ref.SkinTensors(self.joint, self.weight, self.inv, self.rest, self.J, dtype)

    def problem(self, B):
        # (one position constraint on the root and no constraint data: the skeleton state reads no constraints)
        return capi.Problem(self.rh, B, [0], [])

    def states(self, B, seed):
        """[B, J, 8] float32 from Problem.skeleton_state at random theta, as numpy: the same array goes to both sides."""
        theta, _ = fk.random_inputs(self.rig, B, seed)
        return self.problem(B).skeleton_state(_cuda(theta)).cpu().numpy()


def _one_joint_rig():
    return fk.all_dofs_rig([-1], seed=1)


def _character3_k4():
    joint, weight, rest = ref.hand_skin("character3_k4")
    rig = make_test_character(3)
    return Case(rig, joint, weight, make_test_skin(rig, 1, 1, 0).inverse_bind, rest)


def _heavy():
    rig = make_test_character(3)
    rest = make_test_skin(rig, 1000, 1, 31).rest
    return Case(rig, np.zeros((1000, 1), np.int32), np.ones((1000, 1), np.float32), make_test_skin(rig, 1, 1, 0).inverse_bind, rest)


SHAPES = {
    # name: (case factory, batch)
    "one_joint": (lambda: Case(_one_joint_rig(), [[0]], [[1.0]], None, [[0.3, -0.2, 0.5]]), 2),  # no blending, no reduction
    "character3_k4_b1": (_character3_k4, 1),  # padding, an exact-zero row of state_grad
    "character3_k4_b5": (_character3_k4, 5),
    "one_joint_heavy": (_heavy, 2),  # one wave's strided loop over 16 passes plus the cross-lane tree; other joints exact zeros
    "k8": (lambda: Case.synthetic(make_test_character(24), 300, 8, 41, random_affine=True), 3),  # all eight slots, the full 3 x 4
    "humanoid72": (lambda: Case.synthetic(make_humanoid72(variant="p128", unit=0.01), 2000, 4, 42), 4),  # a spread of list lengths
    "rig300": (lambda: Case.synthetic(make_rig300(unit=0.01), 1500, 4, 43), 2),  # more joints than threads in the posed-affine build
}
for _v in (TILE - 1, TILE, TILE + 1, 63, 64, 65):  # the last partial tile and the last partial wave
    SHAPES[f"edge_v{_v}"] = (lambda v=_v: Case.synthetic(make_test_character(3), v, 2, 50 + v), 3)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _dist(x, x64):
    x, x64 = x.reshape(x.shape[0], -1), x64.reshape(x64.shape[0], -1)
    scale = np.abs(x64).max(axis=1)
    return np.abs(x.astype(np.float64) - x64).max(axis=1) / np.where(scale > 0, scale, 1.0)


def _compare(name, got, want64, want32):
    """got / want64 / want32: dicts of arrays [B, ...] by output name."""
    for key in got:
        d32, dg = _dist(want32[key], want64[key]), _dist(got[key], want64[key])
        _parity[f"{name}/{key}"] = dict(gpu=float(dg.max()), d32=float(d32.max()), bound=float(4 * d32.max()))
        print(f"{name}/{key}: gpu {dg.max():.3e}  d32 {d32.max():.3e}  bound {4 * d32.max():.3e}")
    for key in got:
        assert np.isfinite(got[key]).all(), (name, key)
        p = _parity[f"{name}/{key}"]
        assert p["gpu"] <= p["bound"], (name, key, p)


def _run_gpu(case, state, cot, rest=None):
    st, g = _cuda(state), _cuda(cot)
    r = None if rest is None else _cuda(rest)
    out = case.skin.skin_points(st, r)
    sg, rg = case.skin.skin_points_backward(st, g, r, want_rest_grad=True)
    return dict(out=out.cpu().numpy(), state_grad=sg.cpu().numpy(), rest_grad=rg.cpu().numpy())


def _run_ref(case, state, cot, dtype, rest=None):
    out, sg, rg = ref.vjp_autograd(case.tensors(dtype), state, cot, rest)
    return dict(out=out, state_grad=sg, rest_grad=rg)


def _cot(case, B, seed):
    return np.random.default_rng(seed).normal(size=(B, case.V, 3)).astype(np.float32)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_backward_match_the_reference(torch_cuda, name):
    mk, B = SHAPES[name]
    case = mk()
    state, cot = case.states(B, seed=200 + len(name)), _cot(case, B, 300 + len(name))
    got = _run_gpu(case, state, cot)
    want64 = _run_ref(case, state, cot, torch.float64)
    _compare(name, got, want64, _run_ref(case, state, cot, torch.float32))
    # joints without a non-zero-weight influence: eight exact zeros
    used = np.zeros(case.J, bool)
    used[case.joint[case.weight != 0]] = True
    assert np.all(got["state_grad"][:, ~used] == 0.0) and not np.signbit(got["state_grad"][:, ~used]).any()
    assert np.all(np.abs(got["state_grad"][:, used]).max(axis=2) > 0.0)
    if name.startswith("character3_k4"):
        assert not used[2] and used[:2].all()
    if name == "one_joint_heavy":
        assert used.tolist() == [True, False, False]


def test_one_hot_sweep_gives_the_jacobian(torch_cuda):
    """B = 3V instances share one state, instance i carries the i-th unit cotangent: the stacked state_grad is the 3V x 8J
    Jacobian of the vertices -- every channel and sign on its own."""
    case = Case.synthetic(make_test_character(3), 2, 2, 61, random_affine=True)
    V, J = case.V, case.J
    state1 = case.states(1, seed=62)
    state = np.repeat(state1, 3 * V, 0)
    cot = np.eye(3 * V, dtype=np.float32).reshape(3 * V, V, 3)
    got = _run_gpu(case, state, cot)
    sk = case.tensors(torch.float64)
    jac = torch.autograd.functional.jacobian(lambda s: ref.skin_points(sk, s)[0].reshape(-1), torch.as_tensor(state1.astype(np.float64)))
    jac = jac[:, 0].numpy()  # [3V, J, 8]
    want64 = _run_ref(case, state, cot, torch.float64)
    assert np.abs(want64["state_grad"] - jac).max() <= 1e-12 * np.abs(jac).max()  # (the reference's two ways to the Jacobian agree)
    _compare("one_hot_character3", got, want64, _run_ref(case, state, cot, torch.float32))
    # channel by channel: each of the eight is exercised by the sweep and holds the bound on the Jacobian's scale
    bound = _parity["one_hot_character3/state_grad"]["bound"] * np.abs(jac).max()
    for c in range(8):
        assert np.abs(jac[:, :, c]).max() > 0, c
        assert np.abs(got["state_grad"][:, :, c] - jac[:, :, c]).max() <= bound, c


@pytest.mark.parametrize("name", ["character3_k4_b5", "k8"])
def test_per_instance_rest(torch_cuda, name):
    mk, B = SHAPES[name]
    case = mk()
    state, cot = case.states(B, seed=401), _cot(case, B, 402)
    rest = (case.rest[None] + 0.05 * np.random.default_rng(403).normal(size=(B, case.V, 3))).astype(np.float32)
    got = _run_gpu(case, state, cot, rest)
    _compare(f"{name}_instance_rest", got, _run_ref(case, state, cot, torch.float64, rest), _run_ref(case, state, cot, torch.float32, rest))
    # the skin's own rest repeated B times: the same bits as without rest_dev
    shared = _run_gpu(case, state, cot)
    again = _run_gpu(case, state, cot, np.repeat(case.rest[None], B, 0))
    for key in shared:
        assert np.array_equal(shared[key], again[key]), key
    assert not np.array_equal(shared["out"], got["out"])
    # rest_grad is optional
    sg, rg = case.skin.skin_points_backward(_cuda(state), _cuda(cot), _cuda(rest))
    assert rg is None and np.array_equal(sg.cpu().numpy(), got["state_grad"])


def test_non_finite_state_behind_a_zero_weight_slot(torch_cuda):
    case = _character3_k4()
    B = 3
    state, cot = case.states(B, seed=501), _cot(case, B, 502)
    base = _run_gpu(case, state, cot)
    bad = state.copy()
    bad[:, 2] = np.nan  # joint 2 is named by zero-weight slots only
    bad[1, 2] = np.inf
    got = _run_gpu(case, bad, cot)
    for key in base:
        assert np.isfinite(got[key]).all() and np.array_equal(got[key], base[key]), key
    assert np.all(got["state_grad"][:, 2] == 0.0)


def test_a_row_depends_on_its_instance_only(torch_cuda):
    mk, _ = SHAPES["humanoid72"]
    case = mk()
    state, cot = case.states(4, seed=601), _cot(case, 4, 602)
    alone = _run_gpu(case, state[2:3], cot[2:3])
    for pos in (0, 3):
        st, g = state.copy(), cot.copy()
        st[pos], g[pos] = state[2], cot[2]
        out = _run_gpu(case, st, g)
        for key in out:
            assert np.array_equal(out[key][pos], alone[key][0]), (key, pos)
    again = _run_gpu(case, st, g)  # ... nor on the run
    for key in out:
        assert np.array_equal(out[key], again[key]), key


@pytest.mark.parametrize("rig_name", ["chain24", "humanoid72"])
def test_end_to_end_with_the_skeleton_state(torch_cuda, rig_name):
    """theta -> state -> vertices and back, one kernel per stage in each direction."""
    rig = make_test_character(24) if rig_name == "chain24" else make_humanoid72(variant="p128", unit=0.01)
    case = Case.synthetic(rig, 400, 4, 71)
    B = 3
    theta, _ = fk.random_inputs(rig, B, seed=72)
    cot = _cot(case, B, 73)
    pb = case.problem(B)
    th = _cuda(theta).requires_grad_(True)
    verts = mauto.skin_points(case.skin, mauto.skeleton_state(pb, th))
    assert verts.grad_fn is not None
    (verts * _cuda(cot)).sum().backward()

    def chain(dtype):
        rt, sk = fk.RigTensors(rig, dtype), case.tensors(dtype)
        x = torch.as_tensor(theta, dtype=dtype).clone().requires_grad_(True)
        v = ref.skin_points(sk, fk.skeleton_state(rt, x))
        (v * torch.as_tensor(cot, dtype=dtype)).sum().backward()
        return dict(vertices=v.detach().numpy(), theta_grad=x.grad.numpy())

    _compare(f"end_to_end_{rig_name}", dict(vertices=verts.detach().cpu().numpy(), theta_grad=th.grad.cpu().numpy()), chain(torch.float64), chain(torch.float32))
    # without requires_grad: the plain forward, no graph node
    st = pb.skeleton_state(_cuda(theta))
    plain = mauto.skin_points(case.skin, st)
    assert plain.grad_fn is None and torch.equal(plain, verts.detach())
    with torch.no_grad():
        assert mauto.skin_points(case.skin, st.clone().requires_grad_(True)).grad_fn is None
    # per-instance rest as a tensor requiring grad: its gradient is the rest-gradient kernel's
    rest = _cuda(np.repeat(case.rest[None], B, 0)).requires_grad_(True)
    st_leaf = st.clone().requires_grad_(True)
    (mauto.skin_points(case.skin, st_leaf, rest) * _cuda(cot)).sum().backward()
    sg, rg = case.skin.skin_points_backward(st, _cuda(cot), rest.detach(), want_rest_grad=True)
    assert torch.equal(st_leaf.grad, sg) and torch.equal(rest.grad, rg)


def test_refusals_touch_no_output(torch_cuda):
    case = _character3_k4()
    B = 2
    state, cot = case.states(B, seed=801), _cot(case, B, 802)
    st, g = _cuda(state), _cuda(cot)
    out = torch.full((B, case.V, 3), -7.25, device="cuda")
    sgrad = torch.full((B, case.J, 8), -7.25, device="cuda")
    rgrad = torch.full((B, case.V, 3), -7.25, device="cuda")
    L, null, p = capi.lib(), C.c_void_p(0), lambda t: C.c_void_p(t.data_ptr())
    h, stream = case.skin._h, capi._stream_ptr()
    for args in ((null, B, p(st), null, p(out)), (h, B, null, null, p(out)), (h, B, p(st), null, null), (h, 0, p(st), null, p(out)), (h, -1, p(st), null, p(out))):
        assert L.mmx_skin_points(*args, stream) == MMX_ERR_INVALID_ARGUMENT, args
    for args in ((null, B, p(st), null, p(g), p(sgrad), p(rgrad)), (h, B, null, null, p(g), p(sgrad), p(rgrad)), (h, B, p(st), null, null, p(sgrad), p(rgrad)),
                 (h, B, p(st), null, p(g), null, p(rgrad)), (h, 0, p(st), null, p(g), p(sgrad), p(rgrad))):  # fmt: skip
        assert L.mmx_skin_points_backward(*args, stream) == MMX_ERR_INVALID_ARGUMENT, args
    ho, hs, hr = np.full((B, case.V, 3), -7.25, np.float32), np.full((B, case.J, 8), -7.25, np.float32), np.full((B, case.V, 3), -7.25, np.float32)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    for args in ((null, B, hp(state), null, hp(ho)), (h, B, null, null, hp(ho)), (h, B, hp(state), null, null), (h, 0, hp(state), null, hp(ho))):
        assert L.mmx_skin_points_host(*args) == MMX_ERR_INVALID_ARGUMENT, args
    for args in ((null, B, hp(state), null, hp(cot), hp(hs), hp(hr)), (h, B, null, null, hp(cot), hp(hs), hp(hr)), (h, B, hp(state), null, null, hp(hs), hp(hr)),
                 (h, B, hp(state), null, hp(cot), null, hp(hr)), (h, 0, hp(state), null, hp(cot), hp(hs), hp(hr))):  # fmt: skip
        assert L.mmx_skin_points_backward_host(*args) == MMX_ERR_INVALID_ARGUMENT, args
    torch.cuda.synchronize()
    for t in (out, sgrad, rgrad):
        assert torch.all(t == -7.25).item()
    assert all(np.all(a == -7.25) for a in (ho, hs, hr))
    # the host forms compute what the device forms do
    want = _run_gpu(case, state, cot)
    assert L.mmx_skin_points_host(h, B, hp(state), null, hp(ho)) == 0 and np.array_equal(ho, want["out"])
    assert L.mmx_skin_points_backward_host(h, B, hp(state), null, hp(cot), hp(hs), hp(hr)) == 0
    assert np.array_equal(hs, want["state_grad"]) and np.array_equal(hr, want["rest_grad"])
    hs[:] = -7.25
    rest = np.repeat(case.rest[None], B, 0)
    assert L.mmx_skin_points_backward_host(h, B, hp(state), hp(rest), hp(cot), hp(hs), null) == 0 and np.array_equal(hs, want["state_grad"])
    assert L.mmx_skin_num_vertices(h) == case.V


def test_create_refusals(torch_cuda):
    rig = make_test_character(3)
    rh = capi.RigHandle(rig, 0)
    joint, weight, rest = ref.hand_skin("character3_k4")
    inv = make_test_skin(rig, 1, 1, 0).inverse_bind
    L = capi.lib()

    def create(joint=joint, weight=weight, inv=inv, rest=rest, V=None, K=None, rig_h=rh._h, null_out=False):
        d, keep = capi._skin_desc(joint, weight, inv, rest)
        if V is not None:
            d.num_vertices = V
        if K is not None:
            d.max_influences = K
        h = C.c_void_p(0)
        rc = L.mmx_skin_create(rig_h, C.byref(d), None if null_out else C.byref(h))
        if rc == 0:
            L.mmx_skin_destroy(h)
        else:
            assert not h.value
        return rc

    assert create() == 0 and create(inv=None) == 0
    bad_joint = joint.copy()
    bad_joint[0, 3] = 3  # a zero-weight slot
    nan = lambda a, i: np.where(np.arange(a.size).reshape(a.shape) == i, np.nan, a).astype(np.float32)
    for kw in (dict(joint=bad_joint), dict(joint=-joint - 1), dict(V=0), dict(K=0), dict(K=9), dict(weight=nan(weight, 2)),
               dict(weight=np.where(weight == np.float32(0.7), np.float32(np.inf), weight)), dict(inv=nan(inv, 17)), dict(rest=nan(rest, 4)), dict(rest=None),
               dict(rig_h=C.c_void_p(0)), dict(null_out=True)):  # fmt: skip
        assert create(**kw) == MMX_ERR_INVALID_ARGUMENT, list(kw)
    d = _abi.SkinDesc(5, 4, _abi.c_int32_p(), _abi.c_float_p(), _abi.c_float_p(), _abi.c_float_p())
    h = C.c_void_p(0)
    assert L.mmx_skin_create(rh._h, C.byref(d), C.byref(h)) == MMX_ERR_INVALID_ARGUMENT
    assert L.mmx_skin_create(rh._h, None, C.byref(h)) == MMX_ERR_INVALID_ARGUMENT
    # a rig whose posed affines (48 bytes per joint) exceed a workgroup's 160 KB: a root with 3499 children
    big = fk.make_rig([-1] + [0] * 3499, [(0, 3, 0, 1.0)], 1, seed=7)
    with pytest.raises(capi.MmxError) as e:
        capi.Skin(capi.RigHandle(big, 0), [[0]], [[1.0]], None, [[0.0, 0.0, 0.0]])
    assert e.value.code == MMX_ERR_UNSUPPORTED and "LDS budget" in str(e.value), str(e.value)


def test_replays_from_a_captured_graph(torch_cuda):
    """Forward, then backward with the rest gradient, on one stream: a linear chain of three kernel nodes."""
    mk, B = SHAPES["humanoid72"]
    case = mk()
    ins = [(case.states(B, seed=s), _cot(case, B, s + 1)) for s in (901, 903)]
    eager = [_run_gpu(case, s, g) for s, g in ins]  # (also the warm-up)
    st, g = _cuda(ins[0][0]), _cuda(ins[0][1])
    out, rg = torch.zeros((B, case.V, 3), device="cuda"), torch.zeros((B, case.V, 3), device="cuda")
    sg = torch.zeros((B, case.J, 8), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            case.skin.skin_points(st, out=out)
            case.skin.skin_points_backward(st, g, state_grad=sg, rest_grad=rg)
    torch.cuda.current_stream().wait_stream(side)
    for k in (0, 1, 0):
        st.copy_(_cuda(ins[k][0]))
        g.copy_(_cuda(ins[k][1]))
        for t in (out, sg, rg):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, t in (("out", out), ("state_grad", sg), ("rest_grad", rg)):
            assert np.array_equal(t.cpu().numpy(), eager[k][key]), (k, key)
