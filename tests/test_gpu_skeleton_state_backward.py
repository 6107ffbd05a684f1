"""mmx_eval_skeleton_state_backward on the GPU against the float64 reference's autograd gradient
(tests/skeleton_state_reference.py, checked on its own in tests/test_skeleton_state_reference.py).

Distance (tests 1, 2, 5, 7): max|g_gpu - g_ref64| / max|g_ref64| per instance.  Yardstick: the same reference run in float32
on the CPU, whose distance d32 from the float64 run is computed here for the same inputs; the GPU must stay within 4 x the
largest d32 over the test's instances (the factor covers the different summation order: tree sums over DFS ranges instead of
a chain of per-level accumulations).  Inputs: rotations uniform in +-1 rad, translations +-0.2, scales +-0.3, standard-normal
cotangents on all eight channels, fixed seeds.

Measured on an MI355X (largest distance over the instances, gpu | d32 | bound = 4 x d32; profiles/state_backward_parity.json):
    one-hot sweep, character3   3.12e-7 | 2.24e-7 | 8.97e-7        star20            2.67e-7 | 3.13e-7 | 1.25e-6
    joint1_all_dofs             1.11e-7 | 3.18e-8 | 1.27e-7        chain24           1.67e-7 | 2.43e-7 | 9.74e-7
    character3_b1               1.13e-7 | 1.58e-7 | 6.33e-7        humanoid72_p128   3.37e-7 | 2.67e-7 | 1.07e-6
    character3_b5               9.14e-8 | 1.34e-7 | 5.35e-7        rig300            5.04e-7 | 3.27e-7 | 1.31e-6
    chain15                     6.62e-7 | 6.78e-7 | 2.71e-6        table_rig         2.67e-7 | 2.42e-7 | 9.69e-7
    chain16                     4.72e-7 | 6.05e-7 | 2.42e-6        instance rig      2.29e-7 | 3.55e-7 | 1.42e-6
    chain17                     7.95e-7 | 3.59e-7 | 1.44e-6        autograd loss     1.79e-7 | 4.62e-7 | 1.85e-6

The all-dof chains are where the kernel's forward kinematics matters.  With blockFk as the solves run it, chain16 measured 3.51e-6
on one instance (above its bound) and chain15 / chain17 1.3e-6: blockFk builds every LOCAL quaternion in single precision
(|q_l| = 1 +- 5e-8) and composes the world transforms exactly (in double), so the world quaternion's norm is the product of the
local norms -- 1 - 7.8e-7 by joint 15 of that instance, where a float32 chain that rounds after every level stays within
2.6e-7.  A quaternion of norm rho rotates v into (1 - rho^2) v + rho^2 R v, so lever arms and rotation axes below such a joint
are off by 1 - rho^2 = 1.6e-6 relative, and with them every rotation derivative (the channel formulas in float64 on that state
gave the same 4.0e-6).  The backward kernel therefore renormalises each local quaternion in double before the composition
(blockFk's kUnitLocal, used by this kernel alone); the figures above are with it.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import autograd as mauto
from momentum_amd import capi, make_humanoid72, make_rig300, make_test_character
from tests import skeleton_state_reference as ref

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT, MMX_ERR_UNSUPPORTED = 1, 4

SHAPES = {
    # name: (rig factory, batch, what it probes)
    "joint1_all_dofs": (lambda: ref.all_dofs_rig([-1], seed=1), 4),  # no tree
    "character3_b1": (lambda: make_test_character(3), 1),  # smallest real tree, batch of one
    "character3_b5": (lambda: make_test_character(3), 5),
    "chain15": (lambda: ref.all_dofs_rig(ref.chain(15), seed=2), 3),  # the 16-row tile edge of the tree sums
    "chain16": (lambda: ref.all_dofs_rig(ref.chain(16), seed=3), 3),
    "chain17": (lambda: ref.all_dofs_rig(ref.chain(17), seed=4), 3),
    "star20": (lambda: ref.all_dofs_rig([-1] + [0] * 20, seed=5), 3),  # many disjoint subtrees
    "chain24": (lambda: make_test_character(24), 3),  # depth beyond the jump rounds of small rigs
    "humanoid72_p128": (lambda: make_humanoid72(variant="p128", unit=0.01), 4),  # shared parameters
    "rig300": (lambda: make_rig300(unit=0.01), 3),  # more joints than threads: phases C and F take a second pass
    "table_rig": (ref.table_rig, 3),  # table order, zero columns, non-zero pt_offsets
}
_parity = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    """MMX_PARITY_OUT=<file>: the measured distances of this run as JSON (how profiles/state_backward_parity.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _parity:
        with open(out, "w") as f:
            json.dump(dict(unit="max|g - g_ref64| / max|g_ref64| per instance, largest over the instances; bound = 4 x d32", shapes=_parity), f, indent=1)


def _problem(rig, B):
    # (one position constraint on the root and no constraint data: neither direction of the skeleton state reads constraints)
    return capi.Problem(capi.RigHandle(rig, 0), B, [0], [])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _dist(g, g64):
    scale = np.abs(g64).max(axis=1)
    return np.abs(g.astype(np.float64) - g64).max(axis=1) / np.where(scale > 0, scale, 1.0)


def _check_against_reference(name, rig, theta, cot, got, offset=None, pre=None):
    g64 = ref.vjp_autograd(ref.RigTensors(rig), theta, cot, offset, pre)
    g32 = ref.vjp_autograd(ref.RigTensors(rig, torch.float32), theta, cot, offset, pre)
    d32, dg = _dist(g32, g64), _dist(got, g64)
    _parity[name] = dict(gpu=float(dg.max()), d32=float(d32.max()), bound=float(4 * d32.max()))
    print(f"{name}: gpu {dg.max():.3e}  d32 {d32.max():.3e}  bound {4 * d32.max():.3e}")
    assert np.isfinite(got).all()
    assert dg.max() <= 4 * d32.max(), (name, dg, d32)
    return g64


def test_one_hot_sweep_gives_the_state_jacobian(torch_cuda):
    """B = 8J instances share one theta, instance k carries the k-th unit cotangent: the result, stacked, is the 8J x P
    Jacobian of the state -- every channel and sign on its own."""
    rig = make_test_character(3)
    J, P = rig.num_joints, rig.num_params
    theta1, _ = ref.random_inputs(rig, 1, seed=101)
    theta = np.repeat(theta1, 8 * J, 0)
    cot = np.eye(8 * J, dtype=np.float32).reshape(8 * J, J, 8)
    pb = _problem(rig, 8 * J)
    got = pb.skeleton_state_backward(_cuda(theta), _cuda(cot)).cpu().numpy()
    rt = ref.RigTensors(rig)
    jac = torch.autograd.functional.jacobian(lambda x: ref.skeleton_state(rt, x)[0].reshape(-1), torch.as_tensor(theta1.astype(np.float64)))[:, 0].numpy()
    g64 = _check_against_reference("one_hot_character3", rig, theta, cot, got)
    assert np.abs(g64 - jac).max() <= 1e-12  # (the reference's two ways to the Jacobian agree)


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_cotangents_match_the_reference(torch_cuda, name):
    mk, B = SHAPES[name]
    rig = mk()
    theta, cot = ref.random_inputs(rig, B, seed=200 + len(name))
    pb = _problem(rig, B)
    got = pb.skeleton_state_backward(_cuda(theta), _cuda(cot)).cpu().numpy()
    _check_against_reference(name, rig, theta, cot, got)


def test_structure_zero_columns_mask_pruning_and_leaf_cotangent(torch_cuda):
    rig = ref.table_rig()
    B = 3
    theta, cot = ref.random_inputs(rig, B, seed=301)
    pb = _problem(rig, B)
    th, g = _cuda(theta), _cuda(cot)
    base = pb.skeleton_state_backward(th, g).cpu().numpy()
    assert np.all(base[:, 3] == 0.0) and not np.signbit(base[:, 3]).any()  # parameter 3 drives nothing: an exact zero
    assert np.all(base[:, [0, 1, 2, 4, 5, 6, 7]] != 0.0)
    # the enabled mask and joint pruning are not read: the same bits
    mask = np.ones(rig.num_params, np.uint8)
    mask[[0, 2, 5]] = 0
    pb.set_enabled(mask)
    assert np.array_equal(pb.skeleton_state_backward(th, g).cpu().numpy(), base)
    pb.set_joint_pruning(False)
    assert np.array_equal(pb.skeleton_state_backward(th, g).cpu().numpy(), base)
    # a cotangent on the leaf joint 2 alone (chain 0 - 1 - 2): parameters that drive only joints 3 and 4 get exact zeros
    leaf = np.zeros_like(cot)
    leaf[:, 2] = cot[:, 2]
    out = pb.skeleton_state_backward(th, _cuda(leaf)).cpu().numpy()
    assert np.all(out[:, 6] == 0.0) and np.all(out[:, 3] == 0.0)  # parameter 6: ty of joint 4 only
    assert np.all(out[:, [1, 2, 4, 5, 7]] != 0.0)  # joint 2's own rz (two parameters) and the root's dofs
    # ... and parameter 0 (joints 1, 3, 4) sees it through joint 1 only
    assert np.all(out[:, 0] != 0.0)


def test_a_row_depends_on_its_instance_only(torch_cuda):
    rig = make_humanoid72(variant="p128", unit=0.01)
    theta, cot = ref.random_inputs(rig, 130, seed=401)
    i = 77
    th_i, g_i = theta[i : i + 1], cot[i : i + 1]
    alone = _problem(rig, 1).skeleton_state_backward(_cuda(th_i), _cuda(g_i)).cpu().numpy()[0]
    pb = _problem(rig, 130)
    for pos in (0, 129):
        th, g = theta.copy(), cot.copy()
        th[pos], g[pos] = th_i[0], g_i[0]
        out = pb.skeleton_state_backward(_cuda(th), _cuda(g)).cpu().numpy()
        assert np.array_equal(out[pos], alone), pos
    assert np.array_equal(pb.skeleton_state_backward(_cuda(th), _cuda(g)).cpu().numpy(), out)  # ... nor on the run


def test_per_instance_rig(torch_cuda):
    rig = make_humanoid72(variant="p128", unit=0.01)
    B = 4
    theta, cot = ref.random_inputs(rig, B, seed=501)
    scale = np.array([0.8, 1.0, 1.15, 1.3], np.float32)
    offset = (scale[:, None, None] * rig.translation_offset[None]).astype(np.float32)
    pb = _problem(rig, B)
    pb.set_instance_rig(translation_offset=offset)
    got = pb.skeleton_state_backward(_cuda(theta), _cuda(cot)).cpu().numpy()
    _check_against_reference("humanoid72_instance_rig", rig, theta, cot, got, offset=offset)
    shared = _problem(rig, B).skeleton_state_backward(_cuda(theta), _cuda(cot)).cpu().numpy()
    assert np.array_equal(got[1], shared[1]) and not np.array_equal(got[0], shared[0])


def test_refusals_touch_no_output(torch_cuda):
    rig = make_test_character(3)
    B = 2
    pb = _problem(rig, B)
    theta, cot = ref.random_inputs(rig, B, seed=601)
    th, g = _cuda(theta), _cuda(cot)
    out = torch.full((B, rig.num_params), -7.25, device="cuda")
    L, null, p = capi.lib(), C.c_void_p(0), lambda t: C.c_void_p(t.data_ptr())
    stream = capi._stream_ptr()
    for args in ((null, p(g), p(out)), (p(th), null, p(out)), (p(th), p(g), null)):
        assert L.mmx_eval_skeleton_state_backward(pb._h, *args, stream) == MMX_ERR_INVALID_ARGUMENT
    assert L.mmx_eval_skeleton_state_backward(null, p(th), p(g), p(out), stream) == MMX_ERR_INVALID_ARGUMENT
    hth, hg, ho = theta.copy(), cot.copy(), np.full((B, rig.num_params), -7.25, np.float32)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    for args in ((null, hp(hg), hp(ho)), (hp(hth), null, hp(ho)), (hp(hth), hp(hg), null)):
        assert L.mmx_eval_skeleton_state_backward_host(pb._h, *args) == MMX_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.all(out == -7.25).item() and np.all(ho == -7.25)
    # the host form computes what the device form does
    assert L.mmx_eval_skeleton_state_backward_host(pb._h, hp(hth), hp(hg), hp(ho)) == 0
    assert np.array_equal(ho, pb.skeleton_state_backward(th, g).cpu().numpy())


def test_rig_beyond_the_lds_budget_is_refused(torch_cuda):
    """A root with 1023 children: the tables of 1024 joints need more than a workgroup's 160 KB."""
    big = ref.make_rig([-1] + [0] * 1023, [(j, 3, j, 1.0) for j in range(1024)], 1024, seed=7)
    pbig = _problem(big, 1)
    out = torch.full((1, 1024), -7.25, device="cuda")
    with pytest.raises(capi.MmxError) as e:
        pbig.skeleton_state_backward(torch.zeros((1, 1024), device="cuda"), torch.ones((1, 1024, 8), device="cuda"), out=out)
    assert e.value.code == MMX_ERR_UNSUPPORTED and "LDS budget" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert torch.all(out == -7.25).item()


def _loss(st, t_target, q_target):
    return ((st[..., :3] - t_target) ** 2).sum() + ((st[..., 3:7] * q_target).sum(-1) ** 2).sum() + st[..., 7].sum()


def test_autograd_function(torch_cuda):
    rig = make_humanoid72(variant="p128", unit=0.01)
    B = 4
    theta, cot = ref.random_inputs(rig, B, seed=701)
    t_target = 0.3 * cot[..., :3]
    q_target = cot[..., 3:7] / np.linalg.norm(cot[..., 3:7], axis=-1, keepdims=True)
    pb = _problem(rig, B)
    th = _cuda(theta).requires_grad_(True)
    st = mauto.skeleton_state(pb, th)
    assert st.grad_fn is not None
    _loss(st, _cuda(t_target), _cuda(q_target)).backward()
    # the same cotangent through a direct call: the same bits
    leaf = pb.skeleton_state(_cuda(theta)).requires_grad_(True)
    assert torch.equal(leaf.detach(), st.detach())
    _loss(leaf, _cuda(t_target), _cuda(q_target)).backward()
    direct = pb.skeleton_state_backward(_cuda(theta), leaf.grad.contiguous())
    assert torch.equal(th.grad, direct)
    # ... and the reference's gradient of the same loss

    def ref_grad(dtype):
        rt = ref.RigTensors(rig, dtype)
        x = torch.as_tensor(theta, dtype=dtype).clone().requires_grad_(True)
        _loss(ref.skeleton_state(rt, x), torch.as_tensor(t_target, dtype=dtype), torch.as_tensor(q_target, dtype=dtype)).backward()
        return x.grad.numpy()

    g64, g32 = ref_grad(torch.float64), ref_grad(torch.float32)
    d32, dg = _dist(g32, g64), _dist(th.grad.cpu().numpy(), g64)
    _parity["autograd_loss_humanoid72"] = dict(gpu=float(dg.max()), d32=float(d32.max()), bound=float(4 * d32.max()))
    print(f"autograd loss: gpu {dg.max():.3e}  d32 {d32.max():.3e}")
    assert dg.max() <= 4 * d32.max(), (dg, d32)
    # without requires_grad: no graph node
    assert mauto.skeleton_state(pb, _cuda(theta)).grad_fn is None
    with torch.no_grad():
        assert mauto.skeleton_state(pb, th).grad_fn is None


def test_replays_from_a_captured_graph(torch_cuda):
    rig = make_humanoid72(variant="p128", unit=0.01)
    B = 16
    pb = _problem(rig, B)
    ins = [ref.random_inputs(rig, B, seed=s) for s in (801, 802)]
    eager = [pb.skeleton_state_backward(_cuda(t), _cuda(g)).cpu().numpy() for t, g in ins]  # (also the warm-up: the rig's tables)
    th, g, out = _cuda(ins[0][0]), _cuda(ins[0][1]), torch.zeros((B, rig.num_params), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pb.skeleton_state_backward(th, g, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for k in (0, 1, 0):
        th.copy_(_cuda(ins[k][0]))
        g.copy_(_cuda(ins[k][1]))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eager[k]), k
