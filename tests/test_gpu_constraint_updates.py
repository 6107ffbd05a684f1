"""A handle whose constraints are set again and again must compute what a fresh handle given only the latest data computes.

mmx_problem_set_constraints and mmx_problem_set_instance_parents compare every request with what the last accepted one left
and rebuild the derived tables (solve list, limit tables, tile structure, live joints) only when the structure differs; a
wrong "unchanged" would solve with stale tables, silently.  One handle is walked through a sequence built so that every
branch of that comparison is taken -- payload only, limits, the passive limit type (no row, no rebuild), the model-parameter
block, a joint block's payload / loss / one joint, the second joints of a pair block alone, an ellipsoid limit and one of its
values, everything dropped -- with two refused requests in the middle, which must leave the handle as it was.  After every
step the Jacobian, the residual, the error and a 3-iteration solve (default route and explicit-Jacobian route) are compared
with a fresh handle's, bit for bit: the reference is the library itself, so there is no tolerance.  Once with host arrays
(copied by the library), once with device tensors (borrowed)."""
import numpy as np
import pytest

from momentum_amd import _abi, capi, make_test_character
from momentum_amd._abi import EllipsoidLimit, GnOptions, JointBlock, ParameterLimit

pytestmark = pytest.mark.gpu
B = 3
POS_PARENT = np.array([5, 11, 17, 23], np.int32)
ORI_PARENT = np.array([8, 20], np.int32)
MMX_ERR_INVALID_ARGUMENT, MMX_ERR_UNSUPPORTED = 1, 4  # include/mmx.h


def _payload(seed):
    """Position / orientation payload of one step (host arrays)."""
    rng = np.random.default_rng(seed)
    Kp, Ko = len(POS_PARENT), len(ORI_PARENT)

    def q():
        v = rng.normal(size=(B, Ko, 4))
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    return [rng.uniform(-0.2, 0.2, (B, Kp, 3)), rng.uniform(-3.0, 3.0, (B, Kp, 3)) + POS_PARENT[None, :, None] * np.array([0.0, 0.8, 0.0]),
            rng.uniform(0.5, 2.0, (B, Kp)), q(), q(), rng.uniform(0.5, 2.0, (B, Ko))]  # fmt: skip


def _plane(seed, parent, loss=(2.0, 1.0)):
    rng = np.random.default_rng(seed)
    K = len(parent)
    n = rng.normal(size=(B, K, 3))
    return JointBlock(_abi.MMX_JC_PLANE, parent, rng.uniform(0.5, 2.0, (B, K)), n / np.linalg.norm(n, axis=-1, keepdims=True),
                      local_point=rng.uniform(-0.2, 0.2, (B, K, 3)), plane_d=rng.uniform(-1.0, 1.0, (B, K)), function_weight=1.5, loss=loss)  # fmt: skip


def _pair(seed, parent, parent_b):
    rng = np.random.default_rng(seed)
    K = len(parent)
    return JointBlock(_abi.MMX_JC_JOINT_TO_JOINT_DISTANCE, parent, rng.uniform(0.5, 2.0, (B, K)), None, local_point=rng.uniform(-0.2, 0.2, (B, K, 3)),
                      local_dir=rng.uniform(-0.2, 0.2, (B, K, 3)), plane_d=rng.uniform(0.5, 3.0, (B, K)), parent_b=parent_b)  # fmt: skip


def _ellipsoid(scale_x):
    return EllipsoidLimit.make(parent=14, offset=(0.1, 0.2, 0.0), ellipsoid_parent=9, translation=(0.0, 3.0, 0.5), euler_zyx_deg=(10.0, 20.0, 30.0), scale=(scale_x, 2.0, 1.5))


def _steps(P):
    """(name, payload seed, keyword arguments of set_constraints) -- everything as host arrays."""
    rng = np.random.default_rng(7)
    limits = [ParameterLimit.minmax(8, -0.1, 0.1, weight=2.0), ParameterLimit.linear(9, 10, 1.0, 0.1, -1.0, 1.0)]
    passive = ParameterLimit.minmax_joint_passive(3, 3, -0.1, 0.1)
    model = dict(model_target=rng.uniform(-0.3, 0.3, (B, P)), model_weights=rng.uniform(0.1, 1.0, (B, P)), model_function_weight=0.7)
    model2 = dict(model_target=rng.uniform(-0.3, 0.3, (B, P)), model_weights=rng.uniform(0.1, 1.0, (B, P)), model_function_weight=0.7)
    lm = dict(limits=limits + [passive], **model)
    return [
        ("position and orientation only", 1, {}),
        ("two limits added", 2, dict(limits=limits)),
        ("same limits, new weights and payload", 3, dict(limits=limits, limit_function_weight=3.0, pos_function_weight=0.5, ori_function_weight=2.0)),
        ("passive limit appended", 3, dict(limits=limits + [passive], limit_function_weight=3.0, pos_function_weight=0.5, ori_function_weight=2.0)),
        ("model-parameter block added", 4, lm),
        ("plane block added", 5, dict(joint_blocks=[_plane(50, [6, 13, 21])], **lm)),
        ("same block, new payload and a Cauchy loss", 6, dict(joint_blocks=[_plane(51, [6, 13, 21], loss=(0.0, 0.8))], limits=limits + [passive], **model2)),
        ("REFUSED: limit index out of range", 6, dict(limits=limits + [ParameterLimit.minmax(P, -0.1, 0.1)], **model)),
        ("one parent of the block changed", 7, dict(joint_blocks=[_plane(51, [6, 12, 21], loss=(0.0, 0.8))], **lm)),
        ("pair block", 8, dict(joint_blocks=[_plane(51, [6, 12, 21]), _pair(60, [4, 10], [15, 22])], **lm)),
        ("REFUSED: 1025 block constraints", 8, dict(joint_blocks=[_plane(51, [6, 12, 21]), _plane(52, np.arange(1022) % 24)], **lm)),
        ("pair block, second joints changed", 8, dict(joint_blocks=[_plane(51, [6, 12, 21]), _pair(60, [4, 10], [15, 19])], **lm)),
        ("ellipsoid limit added", 9, dict(joint_blocks=[_plane(51, [6, 12, 21]), _pair(60, [4, 10], [15, 19])], ellipsoid_limits=[_ellipsoid(1.0)], **lm)),
        ("one value of the ellipsoid changed", 9, dict(joint_blocks=[_plane(51, [6, 12, 21]), _pair(60, [4, 10], [15, 19])], ellipsoid_limits=[_ellipsoid(1.25)], **lm)),
        ("everything dropped", 1, {}),
    ]  # fmt: skip


def _to_device(torch, device, payload, kw):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    kw = dict(kw)
    for k in ("model_target", "model_weights"):
        if k in kw:
            kw[k] = t(kw[k])
    if "joint_blocks" in kw:
        kw["joint_blocks"] = [JointBlock(k.type, k.parent, t(k.weight), t(k.global_), t(k.local_point), t(k.local_dir), t(k.plane_d), k.function_weight, k.loss,
                                         parent_b=k.parent_b) for k in kw["joint_blocks"]]  # fmt: skip
    return [t(a) for a in payload], kw


def _observe(torch, pb, th0):
    """Everything a caller can see of the problem: J, r, the error, and a short solve on two routes."""
    out = {}
    theta = torch.from_numpy(th0).to(pb.device)
    jac, res, err = pb.eval_jacobian(theta)
    out.update(jac=jac, res=res, err=err)
    opt = GnOptions.make(min_iterations=3, max_iterations=3, threshold=1.0, regularization=0.05)
    for route in ("auto", "explicit_jacobian"):
        pb.set_route(route)
        for k, v in pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt, want_history=True).items():
            out[route + " " + k] = v
    pb.set_route("auto")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), (what, k)


@pytest.fixture(scope="module")
def rig_handle(torch_cuda):
    return capi.RigHandle(make_test_character(24), 0)


@pytest.mark.parametrize("memory", ["host", "device"])
def test_set_again_equals_fresh_handle(torch_cuda, rig_handle, memory):
    torch = torch_cuda
    P = rig_handle.rig.num_params
    th0 = np.random.default_rng(3).uniform(-0.2, 0.2, (B, P)).astype(np.float32)
    pb = capi.Problem(rig_handle, B, POS_PARENT, ORI_PARENT)
    last, refusals = None, 0
    for name, seed, kw in _steps(P):
        payload = _payload(seed)
        if memory == "device":
            payload, kw = _to_device(torch, pb.device, payload, kw)
        if name.startswith("REFUSED"):
            with pytest.raises(capi.MmxError) as e:
                pb.set_constraints(*payload, **kw)
            assert e.value.code == (MMX_ERR_INVALID_ARGUMENT if "limit index" in name else MMX_ERR_UNSUPPORTED), name
            _assert_same(_observe(torch, pb, th0), last, name)  # the handle is as it was
            refusals += 1
            continue
        pb.set_constraints(*payload, **kw)
        fresh = capi.Problem(rig_handle, B, POS_PARENT, ORI_PARENT)
        fresh.set_constraints(*payload, **kw)
        assert pb.M == fresh.M, name
        last = _observe(torch, pb, th0)
        _assert_same(last, _observe(torch, fresh, th0), name)
        fresh.close()
    assert refusals == 2
    pb.close()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_instance_parents_set_again_equal_fresh_handle(torch_cuda, rig_handle, memory):
    torch = torch_cuda
    P = rig_handle.rig.num_params
    th0 = np.random.default_rng(4).uniform(-0.2, 0.2, (B, P)).astype(np.float32)
    payload = _payload(11)
    pos = np.array([[5, 11, 17, 23], [11, 5, 23, 17], [5, 17, 11, 23]], np.int32)
    ori = np.array([[8, 20], [20, 8], [8, 8]], np.int32)
    lists = [
        ("per-instance lists", pos, ori),
        ("same unions, other entries", pos[::-1].copy(), ori[[1, 2, 0]].copy()),
        ("new unions", np.where(pos == 17, 16, pos).astype(np.int32), np.where(ori == 20, 2, ori).astype(np.int32)),
        ("orientation lists only", None, ori),
        ("back to the shared lists", None, None),
    ]
    dev = lambda a: None if a is None else torch.from_numpy(a).to(pb.device)
    pb = capi.Problem(rig_handle, B, POS_PARENT, ORI_PARENT)
    pb.set_constraints(*payload)
    for name, p, o in lists:
        fresh = capi.Problem(rig_handle, B, POS_PARENT, ORI_PARENT)
        fresh.set_constraints(*payload)
        if memory == "device":
            p, o = dev(p), dev(o)
        pb.set_instance_parents(p, o)
        if p is not None or o is not None:
            fresh.set_instance_parents(p, o)
        _assert_same(_observe(torch, pb, th0), _observe(torch, fresh, th0), name)
        fresh.close()
    pb.close()
