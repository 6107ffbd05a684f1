"""GPU checks of the joint-to-joint distance block (include/mmx.h, MMX_JC_JOINT_TO_JOINT_DISTANCE), the first row that walks
two ancestor chains, against the float64 reference of tests/joint_pair_reference.py: the exported J / r / error on small rigs
with every kind of pair, the double route, every single-precision route that carries joint blocks, the columns only a pair
row moves, a fit, switched-off constraints, graph replay, the precision contract, the trust region, refusals, solver2.

Inputs: recipe H (the humanoid; pairs across two branches, inside one hand, ancestor - descendant, one joint twice, limbs to
the trunk) and recipe S (three small random rigs with translation / scale dofs, shared parameters and transform offsets;
ALL pairs a <= b).  The single-precision bound 1e-5 is held on every element: the float32 replay of the reference stays
within 1.1e-6 of its double run on these inputs (tests/test_joint_pair_rows.py asserts 1e-5)."""

import numpy as np
import pytest

from momentum_amd import _abi, capi, solver2
from momentum_amd._abi import (
    MMX_PRECISION_AUTO,
    MMX_PRECISION_F32,
    MMX_PRECISION_F64,
    MMX_PRECISION_MIXED,
    MMX_SOLVE_MIXED,
    MMX_STEP_TRUST_REGION,
    GnOptions,
    JointBlock,
)
from tests import joint_pair_reference as jp

pytestmark = pytest.mark.gpu
LAM, ITERS = jp.LAM, jp.ITERS
PAIR = _abi.MMX_JC_JOINT_TO_JOINT_DISTANCE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m gpu on the MI355X box)")
    return torch


def _dev_block(torch, blk, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    return JointBlock(blk.type, blk.parent, t(blk.weight), t(blk.global_), t(blk.local_point), t(blk.local_dir), t(blk.plane_d),
                      blk.function_weight, blk.loss, parent_b=blk.parent_b)  # fmt: skip


def _set(torch, pb, base, blocks, function_weights=None, device_payload=True):
    B = base.pos_offset.shape[0]
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


def _problem(torch, rig, base, blocks, function_weights=None, device_payload=True):
    pb = capi.Problem(capi.RigHandle(rig, 0), base.pos_offset.shape[0], base.pos_parent, base.ori_parent)
    _set(torch, pb, base, blocks, function_weights, device_payload)
    return pb


def _opts(**kw):
    return GnOptions.make(min_iterations=ITERS, max_iterations=ITERS, threshold=1.0, regularization=LAM, **kw)


def _solve(torch, pb, th0, opt, **kw):
    out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _solve_f64(torch, pb, th0, opt):
    out = pb.solve_f64(torch.from_numpy(th0.astype(np.float64)).to(pb.device), opt)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _cut(blk, idx):
    """the block restricted to the constraints idx"""
    idx = np.asarray(idx)
    return JointBlock(blk.type, blk.parent[idx], blk.weight[:, idx], None, blk.local_point[:, idx], blk.local_dir[:, idx], blk.plane_d[:, idx],
                      blk.function_weight, blk.loss, parent_b=blk.parent_b[idx])  # fmt: skip


def _append(blk, parent, parent_b, weight, offset_a, offset_b, d):
    """the block with one more constraint, the same on every element"""
    B = blk.weight.shape[0]
    col = lambda v, shp: np.broadcast_to(np.asarray(v, np.float32), shp)
    return JointBlock(blk.type, np.append(blk.parent, parent), np.concatenate([blk.weight, col(weight, (B, 1))], axis=1), None,
                      np.concatenate([blk.local_point, col(offset_a, (B, 1, 3))], axis=1), np.concatenate([blk.local_dir, col(offset_b, (B, 1, 3))], axis=1),
                      np.concatenate([blk.plane_d, col(d, (B, 1))], axis=1), blk.function_weight, blk.loss, parent_b=np.append(blk.parent_b, parent_b))  # fmt: skip


@pytest.mark.parametrize("which", range(3))
def test_exported_jacobian_residual_and_error_match_the_reference(torch_cuda, which):
    """Every pair a <= b of a small rig (same joint, ancestor - descendant, two branches; rotation, translation and scale dofs
    above one joint, the other or both) plus one constraint between two coincident points, at theta0 and at a random theta."""
    torch = torch_cuda
    B = 4
    rig, base, blocks, th0, ths = jp.recipe_s(which, B)
    last = rig.num_joints - 1
    sigma_d = np.sqrt(np.float32(1.5)) * np.float32(0.25)
    blk = _append(blocks[0], last, last, 1.5, [0.1, -0.2, 0.05], [0.1, -0.2, 0.05], 0.25)  # coincident points: zero row, residual -sigma d
    pb = _problem(torch, rig, base, [blk])
    assert pb.M == 3 + blk.count == int(capi.lib().mmx_problem_num_rows(pb._h))
    worst = np.zeros(3)
    for theta in (th0, (0.7 * ths[::-1]).astype(np.float32)):
        jac, res, err = pb.eval_jacobian(torch.from_numpy(theta.copy()).to(pb.device))
        jac, res, err = jac.cpu().numpy(), res.cpu().numpy(), err.cpu().numpy()
        for b in range(B):
            J, r, e = jp.full_rows(rig, base.instance(b), [blk.instance(b)], theta[b])
            Jg = jac[b].T
            d = np.array([np.abs(Jg - J).max() / max(1.0, np.abs(J).max()), np.abs(res[b] - r).max() / max(1.0, np.abs(r).max()), abs(err[b] - e) / max(1.0, e)])
            worst = np.maximum(worst, d)
            assert d.max() <= 3e-5, (which, b, d)
            pair = slice(3, 3 + blk.count)
            zero = jp.pair_structural_zeros(rig, blk.instance(b), theta[b])  # no chain passes the column, or a translation above both
            assert np.all(Jg[pair][zero] == 0), (which, b, int((Jg[pair][zero] != 0).sum()))
            assert int(zero.sum()) > blk.count  # (the mask is not empty: most columns miss most pairs)
            assert np.all(Jg[:, np.abs(J).max(axis=0) == 0] == 0)  # structurally zero columns
            assert np.all(Jg[3 + blk.count - 1] == 0) and res[b, 3 + blk.count - 1] == -sigma_d  # the coincident pair
    print(f"rig {which}: worst |J - J_ref|, |r - r_ref|, |e - e_ref| over their scales: {worst[0]:.2e} {worst[1]:.2e} {worst[2]:.2e}")


def test_double_route_matches_the_reference(torch_cuda):
    torch = torch_cuda
    B = 64
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    pb = _problem(torch, rig, base, blocks)
    out = _solve_f64(torch, pb, th0, _opts())
    assert int((out["status"] & 3 != 0).sum()) == 0
    d = jp.rel(out["theta"], jp.solved_h(B))
    print(f"double route vs reference, worst of {B}: {d.max():.2e}")
    assert d.max() <= 1e-9, d.max()


def test_single_precision_routes_match_the_reference(torch_cuda):
    """No element is excluded.  The only widening this test may ever take is 3 x the float32 replay's own distance for an element
    whose replay is itself outside 1e-5 -- on these inputs the replay stays at 1.1e-6, so that is no element."""
    torch = torch_cuda
    B = 64
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    pb = _problem(torch, rig, base, blocks)
    ref = jp.solved_h(B)
    replay = jp.rel(jp.solved_h(B, True).astype(np.float64), ref)
    bound = np.where(replay > 1e-5, 3 * replay, 1e-5)
    print(f"float32 replay vs reference, worst of {B}: {replay.max():.2e}; elements with a widened bound: {int((replay > 1e-5).sum())}")
    assert int((replay > 1e-5).sum()) == 0
    thetas = {}
    for route in ("fused", "wide", "explicit_jacobian"):
        pb.set_route(route)
        out = _solve(torch, pb, th0, _opts())
        assert pb.last_route() == route
        assert int((out["status"] & 3 != 0).sum()) == 0, route
        d = jp.rel(out["theta"], ref)
        print(f"route {route} vs reference, worst of {B}: {d.max():.2e}")
        assert np.all(d <= bound), (route, d.max(), int(np.argmax(d)))
        thetas[route] = out["theta"]
    for route in ("wide", "explicit_jacobian"):
        d = jp.rel(thetas[route], thetas["fused"])
        print(f"route {route} vs fused, worst: {d.max():.2e}")
        assert d.max() <= 1e-5, route
    pb.set_route("auto")
    out = _solve(torch, pb, th0, _opts(precision=MMX_PRECISION_AUTO))
    d = jp.rel(out["theta"], ref)
    print(f"route auto, precision AUTO vs reference, worst: {d.max():.2e}")
    assert np.all(d <= bound), d.max()


def test_columns_only_a_pair_row_moves_are_solved(torch_cuda):
    """Parameters below a B joint that no anchor and no A joint's chain reaches: they are in the system only because of the
    second chain.  Missing B joints in a host list (solve lists, source slots) leave them out or leave them still."""
    torch = torch_cuda
    B = 64
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    pb = _problem(torch, rig, base, blocks)
    split = 3 * base.Kp
    only = []
    for b in (0, 1, B - 1):
        J, _, _ = jp.full_rows(rig, base.instance(b), [blocks[0].instance(b)], th0[b])
        anchor = np.abs(J[:split]).max(axis=0) > 0
        pair = np.abs(J[split:split + blocks[0].count]).max(axis=0) > 0
        only.append(np.flatnonzero(pair & ~anchor))
        assert len(only[-1]) >= 50, len(only[-1])
    solve_list, _, _ = pb.fused_normal_equations(torch.from_numpy(th0.copy()).to(pb.device))
    for cols in only:
        assert set(cols) <= set(int(p) for p in solve_list), sorted(set(cols) - set(int(p) for p in solve_list))
    for route in ("fused", "wide", "explicit_jacobian"):
        pb.set_route(route)
        th = _solve(torch, pb, th0, _opts())["theta"]
        assert pb.last_route() == route
        for b, cols in zip((0, 1, B - 1), only):
            assert np.all(th[b, cols] != th0[b, cols]), (route, b, cols[th[b, cols] == th0[b, cols]])


@pytest.mark.parametrize("which", range(3))
def test_small_rigs_solve(torch_cuda, which):
    torch = torch_cuda
    B = 16
    rig, base, blocks, th0, _ = jp.recipe_s(which, B)
    pb = _problem(torch, rig, base, blocks)
    ref = jp.solved_s(which, B)
    out = _solve(torch, pb, th0, _opts())
    assert int((out["status"] & 3 != 0).sum()) == 0
    d32 = jp.rel(out["theta"], ref)
    out = _solve_f64(torch, pb, th0, _opts())
    assert int((out["status"] & 3 != 0).sum()) == 0
    d64 = jp.rel(out["theta"], ref)
    print(f"rig {which}: route {pb.last_route()} vs reference {d32.max():.2e}, double route {d64.max():.2e}")
    assert d32.max() <= 1e-5, d32
    assert d64.max() <= 1e-9, d64


def test_fit_reaches_the_reference_objective(torch_cuda):
    torch = torch_cuda
    B = 32
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    ref = jp.solved_h(B)
    pb = _problem(torch, rig, base, blocks)
    pb.set_route("fused")
    th = _solve(torch, pb, th0, _opts())["theta"]
    assert pb.last_route() == "fused"
    for b in range(B):
        inst = (base.instance(b), [k.instance(b) for k in blocks])
        e0, e_ref, e_got = (jp.full_rows(rig, *inst, t)[2] for t in (th0[b], ref[b], th[b]))
        assert e_ref <= 1e-2 * e0, (b, e_ref, e0)
        assert abs(e_got - e_ref) <= 1e-6 * e0 + 1e-5 * e_ref, (b, e_got, e_ref, e0)


def test_switched_off_constraints_change_nothing(torch_cuda):
    """A zero constraint weight, a block function weight of 0 and a per-element function-weight column of 0 give results
    bit-identical to the problem without that constraint / block (one-launch route).  The switched-off constraints sit on
    joints the other constraints already use, so the structure of the system is the same with and without them."""
    torch = torch_cuda
    B = 16
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    blk = blocks[0]

    def run(blks, fw=None):
        pb = _problem(torch, rig, base, blks, fw)
        pb.set_route("fused")
        th = _solve(torch, pb, th0, _opts())["theta"]
        assert pb.last_route() == "fused"
        return th

    without = run([blk])
    assert np.array_equal(run([_append(blk, blk.parent[0], blk.parent_b[0], 0.0, [0.01, 0.0, 0.0], [0.0, 0.02, 0.0], 0.1)]), without)
    extra = _cut(blk, [0, 1, 2])
    extra.plane_d = extra.plane_d + 0.1
    off = _cut(extra, [0, 1, 2])
    off.function_weight = 0.0
    assert np.array_equal(run([blk, off]), without)
    fw = np.ones((B, 6), np.float32)
    fw[:, 5] = 0.0
    assert np.array_equal(run([blk, extra], fw), without)
    assert not np.array_equal(run([blk, extra]), without)  # ... and switched on, the second block does pull


@pytest.mark.parametrize("precision", ["f32", "auto"])
def test_pair_solve_replays_from_a_captured_graph(torch_cuda, precision):
    torch = torch_cuda
    B = 64
    rig, base, blocks, th0, ths = jp.recipe_h(B)
    th1 = (0.5 * ths).astype(np.float32)
    pb = _problem(torch, rig, base, blocks)
    pb.set_route("fused")
    opt = _opts(precision=MMX_PRECISION_AUTO if precision == "auto" else MMX_PRECISION_F32)
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


def test_mixed_precision_is_the_double_instantiation(torch_cuda):
    """Today's contract for problems with joint blocks: MMX_PRECISION_MIXED runs the double kernel on every element."""
    torch = torch_cuda
    B = 64
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    pb = _problem(torch, rig, base, blocks)
    a = _solve(torch, pb, th0, _opts(precision=MMX_PRECISION_MIXED))
    d = _solve(torch, pb, th0, _opts(precision=MMX_PRECISION_F64))
    assert np.all(a["status"] & MMX_SOLVE_MIXED == 0)
    assert np.array_equal(a["theta"], d["theta"]) and np.array_equal(a["status"], d["status"])
    assert jp.rel(d["theta"].astype(np.float64), jp.solved_h(B)).max() <= 1e-6  # (theta leaves the double kernel as float32)


def test_trust_region_with_pair_blocks_follows_the_double_trust_region(torch_cuda):
    torch = torch_cuda
    B = 32
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    pb = _problem(torch, rig, base, blocks)
    opt = GnOptions.make(min_iterations=8, max_iterations=8, threshold=1.0, step_rule=MMX_STEP_TRUST_REGION)
    out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt, want_history=True)
    assert pb.last_route() == "wide"
    assert int((out["status"] & 1 != 0).sum()) == 0
    th = out["theta"].cpu().numpy()
    ref = pb.solve_f64(torch.from_numpy(th0.astype(np.float64)).to(pb.device), opt)["theta"].cpu().numpy()
    for b in range(B):
        inst = (base.instance(b), [k.instance(b) for k in blocks])
        e_tr, e_ref = jp.full_rows(rig, *inst, th[b])[2], jp.full_rows(rig, *inst, ref[b])[2]
        assert e_tr <= 1.001 * e_ref + 0.001, (b, e_tr, e_ref)
    h = out["error_history"].cpu().numpy()
    assert np.all(np.diff(h, axis=1) <= 1e-6 * np.abs(h[:, :-1]) + 1e-12)


def test_refusals(torch_cuda):
    torch = torch_cuda
    B = 2
    rig, base, blocks, th0, _ = jp.recipe_h(B)
    blk = blocks[0]
    mk = lambda **kw: JointBlock(**{**dict(type=PAIR, parent=blk.parent, weight=blk.weight, global_=None, local_point=blk.local_point,
                                           local_dir=blk.local_dir, plane_d=blk.plane_d, parent_b=blk.parent_b), **kw})  # fmt: skip
    pb = _problem(torch, rig, base, [blk], device_payload=False)  # global=None is accepted
    rows = 3 * base.Kp + blk.count
    assert int(capi.lib().mmx_problem_num_rows(pb._h)) == rows
    before = _solve(torch, pb, th0, _opts())["theta"]

    def refused(b, code):
        with pytest.raises(capi.MmxError) as ei:
            _set(torch, pb, base, [blk, b], device_payload=False)
        assert ei.value.code == code, str(ei.value)
        # ... before anything was modified: the handle still holds the one-block problem
        assert int(capi.lib().mmx_problem_num_rows(pb._h)) == rows

    bad_b = blk.parent_b.copy()
    bad_b[-1] = rig.num_joints
    refused(mk(parent_b=bad_b), 1)  # MMX_ERR_INVALID_ARGUMENT: second parent out of range
    bad_b[-1] = -1
    refused(mk(parent_b=bad_b), 1)
    bad_a = blk.parent.copy()
    bad_a[0] = rig.num_joints
    refused(mk(parent=bad_a), 1)
    refused(mk(local_dir=None), 1)
    refused(mk(plane_d=None), 1)
    refused(mk(local_point=None), 1)
    for loss in ((1.0, 0.5), (0.0, 1.0), (2.0, 2.0)):
        refused(mk(loss=loss), 4)  # MMX_ERR_UNSUPPORTED
    assert np.array_equal(_solve(torch, pb, th0, _opts())["theta"], before)
    for loss in ((2.0, 1.0), (5.0, 0.0)):  # the default loss, spelled both ways, is taken
        _problem(torch, rig, base, [mk(loss=loss)], device_payload=False)
    # the one-wavefront route keeps refusing joint blocks
    pb.set_route("wave")
    t = torch.from_numpy(th0.copy()).to(pb.device)
    with pytest.raises(capi.MmxError) as ei:
        pb.solve(t, _opts())
    assert ei.value.code == 4, str(ei.value)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), th0)


def test_solver2_pinch(torch_cuda):
    """A thumb-to-index pinch through the solver2 surface: the fingertips end at the target distance."""
    rig = jp.humanoid()
    ch = solver2.Character(rig)
    idx = lambda n: rig.joint_names.index(n)
    thumb, index = idx("thumb3_l"), idx("index3_l")
    tip_t, tip_i = np.array([0.0, 0.01, 0.0], np.float32), np.array([0.0, 0.012, 0.0], np.float32)
    th0 = np.zeros(rig.num_params, np.float32)
    xa, _ = jp.world_points(rig, [thumb], tip_t[None], th0)
    xb, _ = jp.world_points(rig, [index], tip_i[None], th0)
    start = float(np.linalg.norm(xa - xb))
    target = 0.25 * start
    pair = solver2.JointToJointDistanceErrorFunction(ch)
    pair.add_constraint(thumb, tip_t, index, tip_i, target, name="pinch")
    anchor = solver2.PositionErrorFunction(ch)
    wrist = idx("wrist_l")
    xw, _ = jp.world_points(rig, [wrist], np.zeros((1, 3)), th0)
    anchor.add_constraint(wrist, xw[0].astype(np.float32))
    fn = solver2.SkeletonSolverFunction(ch, [pair, anchor])
    opt = solver2.GaussNewtonSolverOptions()
    opt.min_iterations = opt.max_iterations = 10
    opt.regularization = 1e-4
    solver = solver2.GaussNewtonSolver(fn, opt)
    th = np.asarray(solver.solve(th0), np.float64)
    xa, _ = jp.world_points(rig, [thumb], tip_t[None], th)
    xb, _ = jp.world_points(rig, [index], tip_i[None], th)
    got = float(np.linalg.norm(xa - xb))
    print(f"pinch: distance {start:.4f} -> {got:.4f}, target {target:.4f}")
    assert abs(got - target) <= 0.01 * target
