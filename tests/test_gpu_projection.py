"""GPU checks of the projection / distance joint blocks (include/mmx.h ABI 12, MMX_JC_PROJECTION / MMX_JC_DISTANCE) against
the float64 reference of tests/projection_reference.py (the oracle's point rows times df/dx): the exported J and r, the
double route, every single-precision route that carries joint blocks, a keypoint fit, switched-off constraints, graph
replay, refusals, the trust region."""

import numpy as np
import pytest

from momentum_amd import _abi, capi, humanoid72_landmark_joints, make_humanoid72
from momentum_amd._abi import MMX_PRECISION_AUTO, MMX_SOLVE_PRECISION_SUSPECT, MMX_STEP_TRUST_REGION, GnOptions, JointBlock
from tests import projection_reference as pr

pytestmark = pytest.mark.gpu
UNIT = 0.01
LAM, ITERS = 0.05, 6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m gpu on the MI355X box)")
    return torch


@pytest.fixture(scope="module")
def rig():
    return make_humanoid72(unit=UNIT)


def _dev_block(torch, blk, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    return JointBlock(blk.type, blk.parent, t(blk.weight), t(blk.global_), t(blk.local_point), None, t(blk.plane_d), blk.function_weight, blk.loss,
                      t(blk.projection), blk.near_clip)  # fmt: skip


def _problem(torch, rig, base, blocks, function_weights=None, device_payload=True):
    B = base.pos_offset.shape[0]
    pb = capi.Problem(capi.RigHandle(rig, 0), B, base.pos_parent, base.ori_parent)
    dev = pb.device
    if device_payload:
        t = lambda a, shp: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shp)).to(dev)
        gb = [_dev_block(torch, k, dev) for k in blocks]
        fw = None if function_weights is None else t(function_weights, function_weights.shape)
    else:
        t = lambda a, shp: np.ascontiguousarray(a, np.float32).reshape(shp)
        gb, fw = blocks, function_weights
    pb.set_constraints(t(base.pos_offset, (B, base.Kp, 3)), t(base.pos_target, (B, base.Kp, 3)), t(base.pos_weight, (B, base.Kp)),
                       t(base.ori_offset, (B, 0, 4)), t(base.ori_target, (B, 0, 4)), t(base.ori_weight, (B, 0)),
                       joint_blocks=gb, function_weights=fw)  # fmt: skip
    return pb


def _opts(**kw):
    return GnOptions.make(min_iterations=ITERS, max_iterations=ITERS, threshold=1.0, regularization=LAM, **kw)


def _ref_solve(rig, base, blocks, th0, idx):
    return np.stack([pr.gauss_newton(rig, base.instance(b), [k.instance(b) for k in blocks], th0[b], LAM, ITERS) for b in idx])


def _rel(a, b):
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def test_exported_jacobian_and_residual_match_the_reference(torch_cuda, rig):
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 4
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 5, lm, lm, n_cams=2, dist_parents=lm[:4], behind=True)
    pb = _problem(torch, rig, base, blocks)
    rows = 3 * base.Kp + sum(k.rows for k in blocks)
    assert pb.M == rows == int(capi.lib().mmx_problem_num_rows(pb._h))
    jac, res, err = pb.eval_jacobian(torch.from_numpy(th0).to(pb.device))
    jac, res, err = jac.cpu().numpy(), res.cpu().numpy(), err.cpu().numpy()
    clip0 = 3 * base.Kp + 2 * (blocks[0].count - 1)
    for b in range(B):
        J, r, e = pr.full_rows(rig, base.instance(b), [k.instance(b) for k in blocks], th0[b])
        Jg = jac[b].T
        scale = max(1.0, np.abs(J).max())
        assert np.abs(Jg - J).max() <= 3e-5 * scale, (b, np.abs(Jg - J).max())
        assert np.all(Jg[:, np.abs(J).max(axis=0) == 0] == 0)  # structurally zero columns
        assert np.all(Jg[clip0:clip0 + 2] == 0) and np.all(res[b, clip0:clip0 + 2] == 0)  # the clipped constraint's rows
        assert np.abs(res[b] - r).max() <= 3e-5 * max(1.0, np.abs(r).max())
        assert abs(err[b] - e) <= 3e-5 * max(1.0, e)


def test_double_route_matches_the_reference(torch_cuda, rig):
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 256
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 11, lm, lm, n_cams=2, dist_parents=lm[:4], behind=True)
    assert len({blocks[0].global_[b].tobytes() for b in range(B)}) == B  # distinct instances
    pb = _problem(torch, rig, base, blocks)
    th = torch.from_numpy(th0.astype(np.float64)).to(pb.device)
    out = pb.solve_f64(th, _opts())
    assert int((out["status"] & 3 != 0).sum()) == 0
    got = out["theta"].cpu().numpy()
    ref = _ref_solve(rig, base, blocks, th0, range(B))
    assert _rel(got, ref).max() <= 1e-9, _rel(got, ref).max()


def test_single_precision_routes_match_the_reference(torch_cuda, rig):
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 64
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 17, lm, lm, n_cams=2, dist_parents=lm[:4], behind=True)
    pb = _problem(torch, rig, base, blocks)
    ref = _ref_solve(rig, base, blocks, th0, range(B))
    thetas = {}
    for route in ("fused", "wide", "explicit_jacobian"):
        pb.set_route(route)
        out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), _opts())
        assert pb.last_route() == route
        st = out["status"].cpu().numpy()
        assert int((st & 3 != 0).sum()) == 0
        th = out["theta"].cpu().numpy()
        rel = _rel(th, ref)
        ok = (st & MMX_SOLVE_PRECISION_SUSPECT) == 0 if route != "explicit_jacobian" else np.ones(B, bool)
        assert ok.sum() >= B // 2, route
        assert rel[ok].max() <= 1e-5, (route, rel[ok].max())
        thetas[route] = th
    for route in ("wide", "explicit_jacobian"):
        assert _rel(thetas[route], thetas["fused"]).max() <= 1e-5, route
    pb.set_route("auto")
    out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), _opts(precision=MMX_PRECISION_AUTO))
    assert _rel(out["theta"].cpu().numpy(), ref).max() <= 1e-5


def test_keypoint_fit_reaches_the_reference_objective(torch_cuda, rig):
    """2D keypoints of a ground-truth pose through three cameras plus one keypoint behind a camera; the solve starts from a
    perturbed ground truth and lands on the objective the double reference reaches in the same iterations."""
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 32
    base, blocks, _, ths = pr.keypoint_problem(rig, B, 29, lm[:2], lm, n_cams=3, behind=True)
    rng = np.random.default_rng(1)
    th0 = (ths + rng.uniform(-0.1, 0.1, ths.shape)).astype(np.float32)
    pb = _problem(torch, rig, base, blocks)
    pb.set_route("fused")
    out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), _opts())
    assert pb.last_route() == "fused"
    th = out["theta"].cpu().numpy()
    for b in range(B):
        inst = (base.instance(b), [k.instance(b) for k in blocks])
        e0 = pr.full_rows(rig, *inst, th0[b])[2]
        ref = pr.gauss_newton(rig, *inst, th0[b], LAM, ITERS)
        e_ref, e_got = pr.full_rows(rig, *inst, ref)[2], pr.full_rows(rig, *inst, th[b])[2]
        assert e_ref < 1e-2 * e0, (b, e_ref, e0)
        assert abs(e_got - e_ref) <= 1e-6 * e0 + 1e-5 * e_ref, (b, e_got, e_ref, e0)


def test_switched_off_constraints_change_nothing(torch_cuda, rig):
    """A clipped constraint, a zero constraint weight, a block function weight <= 0 and a per-element function-weight
    column of 0 give results bit-identical to the problem without that constraint / block (one-launch route)."""
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 16
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 41, lm, lm, n_cams=2, dist_parents=lm[:4], behind=True)
    proj, dist = blocks
    K = proj.count
    cut = lambda blk, n: JointBlock(blk.type, blk.parent[:n], blk.weight[:, :n], blk.global_[:, :n], blk.local_point[:, :n],
                                    projection=blk.projection[:, :n], near_clip=blk.near_clip)  # fmt: skip

    def run(blks, fw=None):
        pb = _problem(torch, rig, base, blks, fw)
        pb.set_route("fused")
        out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), _opts())
        assert pb.last_route() == "fused"
        return out["theta"].cpu().numpy()

    without = run([cut(proj, K - 1), dist])
    assert np.array_equal(run([proj, dist]), without)  # the last constraint is behind its camera
    zero_w = cut(proj, K)
    zero_w.weight = zero_w.weight.copy()
    zero_w.weight[:, -1] = 0.0
    zero_w.projection = zero_w.projection.copy()
    zero_w.projection[:, -1] = proj.projection[:, 0]  # in front of its camera, weight 0
    assert np.array_equal(run([zero_w, dist]), without)
    base_two = run([cut(proj, K - 1), dist])
    off = JointBlock(dist.type, dist.parent, dist.weight, dist.global_, dist.local_point, plane_d=dist.plane_d + 0.1, function_weight=0.0)
    assert np.array_equal(run([cut(proj, K - 1), dist, off]), base_two)
    on = JointBlock(dist.type, dist.parent, dist.weight, dist.global_, dist.local_point, plane_d=dist.plane_d + 0.1)
    fw = np.ones((B, 7), np.float32)
    fw[:, 6] = 0.0
    assert np.array_equal(run([cut(proj, K - 1), dist, on], fw), base_two)


@pytest.mark.parametrize("precision", ["f32", "auto"])
def test_projection_solve_replays_from_a_captured_graph(torch_cuda, rig, precision):
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 64
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 53, lm, lm, n_cams=2, dist_parents=lm[:4], behind=True)
    _, _, _, ths = pr.keypoint_problem(rig, B, 54, lm[:1], lm[:1], n_cams=1)
    th1 = (0.5 * ths).astype(np.float32)
    pb = _problem(torch, rig, base, blocks)
    pb.set_route("fused")
    opt = _opts(precision=MMX_PRECISION_AUTO if precision == "auto" else _abi.MMX_PRECISION_F32)
    dev = pb.device
    outs = lambda: dict(error=torch.empty((B,), dtype=torch.float64, device=dev), iterations=torch.empty((B,), dtype=torch.int32, device=dev),
                        status=torch.empty((B,), dtype=torch.int32, device=dev))  # fmt: skip

    def eager(th):
        o = outs()
        pb.solve(torch.from_numpy(th.copy()).to(dev), opt, outputs=o)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    ref0, ref1 = eager(th0), eager(th1)
    assert pb.last_route() == "fused"
    theta = torch.from_numpy(th0.copy()).to(dev)
    theta_in = theta.clone()
    go = outs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            theta.copy_(theta_in)
            pb.solve(theta, opt, outputs=go)
    torch.cuda.current_stream().wait_stream(side)
    for th, ref in ((th0, ref0), (th1, ref1), (th0, ref0)):
        theta_in.copy_(torch.from_numpy(th.copy()).to(dev))
        for v in go.values():
            if v is not theta:
                v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in ("theta", "error", "iterations", "status"):
            assert np.array_equal(go[k].cpu().numpy(), ref[k], equal_nan=(k in ("error", "theta"))), (precision, k)


def test_refusals_and_row_count(torch_cuda, rig):
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 2
    base, blocks, _, _ = pr.keypoint_problem(rig, B, 3, lm[:2], lm[:3], n_cams=2, dist_parents=lm[:2])
    pb = _problem(torch, rig, base, blocks, device_payload=False)
    assert int(capi.lib().mmx_problem_num_rows(pb._h)) == 3 * 2 + 2 * 6 + 2
    proj, dist = blocks

    def refused(blks, code):
        with pytest.raises(capi.MmxError) as ei:
            _problem(torch, rig, base, blks, device_payload=False)
        assert ei.value.code == code, str(ei.value)

    nulled = JointBlock(proj.type, proj.parent, proj.weight, proj.global_, proj.local_point, projection=None)
    refused([nulled], 1)  # MMX_ERR_INVALID_ARGUMENT
    for loss in ((1.0, 0.5), (0.0, 1.0), (2.0, 2.0)):
        refused([JointBlock(proj.type, proj.parent, proj.weight, proj.global_, proj.local_point, loss=loss, projection=proj.projection)], 4)
        refused([JointBlock(dist.type, dist.parent, dist.weight, dist.global_, dist.local_point, plane_d=dist.plane_d, loss=loss)], 4)  # UNSUPPORTED
    for nc in (float("nan"), float("inf")):
        refused([JointBlock(proj.type, proj.parent, proj.weight, proj.global_, proj.local_point, projection=proj.projection, near_clip=nc)], 1)
    # the default loss spelled both ways is taken
    _problem(torch, rig, base, [JointBlock(dist.type, dist.parent, dist.weight, dist.global_, dist.local_point, plane_d=dist.plane_d, loss=(5.0, 0.0))],
             device_payload=False)  # fmt: skip


def test_trust_region_with_projection_blocks_follows_the_double_trust_region(torch_cuda, rig):
    torch = torch_cuda
    lm = humanoid72_landmark_joints(rig)
    B = 32
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 61, lm, lm, n_cams=2, dist_parents=lm[:4], behind=True)
    pb = _problem(torch, rig, base, blocks)
    opt = GnOptions.make(min_iterations=8, max_iterations=8, threshold=1.0, step_rule=MMX_STEP_TRUST_REGION)
    out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt, want_history=True)
    assert pb.last_route() == "wide"
    assert int((out["status"] & 1 != 0).sum()) == 0
    th = out["theta"].cpu().numpy()
    ref = pb.solve_f64(torch.from_numpy(th0.astype(np.float64)).to(pb.device), opt)["theta"].cpu().numpy()
    for b in range(B):
        inst = (base.instance(b), [k.instance(b) for k in blocks])
        e_tr, e_ref = pr.full_rows(rig, *inst, th[b])[2], pr.full_rows(rig, *inst, ref[b])[2]
        assert e_tr <= 1.001 * e_ref + 0.001, (b, e_tr, e_ref)
    h = out["error_history"].cpu().numpy()
    assert np.all(np.diff(h, axis=1) <= 1e-6 * np.abs(h[:, :-1]) + 1e-12)
