"""MMX_ROUTE_WAVE: one wavefront per instance (momentum_amd/csrc/mmx_wave.hip), pinned, against the oracle's DOUBLE instantiation.

rel = |theta - theta_f64| / max(|theta_f64|, 1e-3) per instance.  1e-5 is north_star's bound (bench.py PARITY_BOUND); the
input sets are the ones on which the oracle's own float instantiation stays inside it (issue text: 4.6e-7 ... 6.4e-6), so no
instance is exempted.  The fuzz seeds take the existing fuzz test's bound (2e-5, widened to 3 x the float oracle's own distance
only for a seed that exceeds it: at most two seeds may need that)."""
import os
from collections import Counter

import numpy as np
import pytest

from momentum_amd import _abi, capi, make_humanoid72, humanoid72_landmark_joints, make_test_character
from momentum_amd._abi import GnOptions, ParameterLimit
from tests.helpers import make_problem
from tests.test_gpu_fuzz import random_rig
from tests.test_real_rig import fixture_rig

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXED = dict(min_iterations=10, max_iterations=10, threshold=1.0, regularization=0.05)
DRIVER = dict(min_iterations=4, max_iterations=50, threshold=10.0, regularization=0.01)


def _sets():
    glb = fixture_rig(np.load(os.path.join(GOLDEN, "real_rig_character_with_motion.npz"), allow_pickle=True))
    return {
        "glb": (glb, {}),
        "char3": (make_test_character(3), {}),
        "chain24": (make_test_character(24), {}),
        "chain24_offsets_weights": (make_test_character(24), dict(random_offsets=True, weights="random")),
    }


def _all_joints(rig):
    return np.arange(rig.num_joints, dtype=np.int32)


def _problem(torch, rig, cons, B, route="wave", **kw):
    pb = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
    t = lambda a, shp: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shp)).to(pb.device)
    for k in ("function_weights",):
        if kw.get(k) is not None:
            kw[k] = t(kw[k], np.asarray(kw[k]).shape)
    pb.set_constraints(t(cons.pos_offset, (B, cons.Kp, 3)), t(cons.pos_target, (B, cons.Kp, 3)), t(cons.pos_weight, (B, cons.Kp)),
                       t(cons.ori_offset, (B, cons.Ko, 4)), t(cons.ori_target, (B, cons.Ko, 4)), t(cons.ori_weight, (B, cons.Ko)), **kw)  # fmt: skip
    if route is not None:
        pb.set_route(route)
    return pb


def _solve(torch, pb, th0, opt, **kw):
    out = pb.solve(torch.from_numpy(np.ascontiguousarray(th0, np.float32).copy()).to(pb.device), opt, want_history=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _rel(th, ref):
    return np.linalg.norm(th - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-3)


def _check_fixed(out, ref, th0, en=None, bound=1e-5):
    rel = _rel(out["theta"], ref["theta"])
    print("worst rel %.3e" % rel.max())
    assert np.all(rel <= bound), (rel.max(), int((rel > bound).sum()))
    assert np.array_equal(out["iterations"], ref["iterations"])
    assert np.array_equal(out["status"] & 3, ref["status"])
    h, href = out["error_history"], ref["error_history"]
    assert np.abs(h - href).max() <= 1e-4 * max(1.0, np.abs(href).max())
    if en is not None:
        assert np.all(out["theta"][:, en == 0] == th0[:, en == 0])


@pytest.mark.parametrize("name", sorted(_sets()))
def test_fixed_iteration_count(torch_cuda, orc, name):
    rig, kw = _sets()[name]
    B = 256
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3, **kw)
    opt = GnOptions.make(**FIXED)
    pb = _problem(torch_cuda, rig, cons, B)
    out = _solve(torch_cuda, pb, th0, opt)
    assert pb.last_route() == "wave"
    ref = orc.solve_batch(rig, cons, th0, opt, dtype="f64")
    _check_fixed(out, ref, th0)


@pytest.mark.parametrize("name,line_search", [(n, 2) for n in sorted(_sets())] + [("chain24_offsets_weights", 1)])
def test_driver_defaults(torch_cuda, orc, name, line_search):
    rig, kw = _sets()[name]
    B = 256
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3, **kw)
    opt = GnOptions.make(do_line_search=line_search, **DRIVER)
    pb = _problem(torch_cuda, rig, cons, B)
    out = _solve(torch_cuda, pb, th0, opt)
    assert pb.last_route() == "wave"
    ref = orc.solve_batch(rig, cons, th0, opt, dtype="f64")
    ref32 = orc.solve_batch(rig, cons, th0, opt, dtype="f32")
    for tag, it in (("oracle f64", ref["iterations"]), ("oracle f32", ref32["iterations"]), ("gpu wave", out["iterations"])):
        print(tag, "iterations:", sorted(Counter(int(x) for x in it).items()))
    rel = _rel(out["theta"], ref["theta"])
    print("worst rel %.3e (float oracle %.3e)" % (rel.max(), _rel(ref32["theta"], ref["theta"]).max()))
    assert np.all(rel <= 1e-5), (rel.max(), int((rel > 1e-5).sum()))
    assert np.array_equal(out["status"] & 3, ref["status"])
    assert np.all((out["iterations"] >= 4) & (out["iterations"] <= 50))
    assert np.abs(out["error"] - ref["error"]).max() <= 1e-4 * max(1.0, np.abs(ref["error"]).max())


def test_baseline_config0_fixture(torch_cuda):
    """BASELINE configs[0] as committed: the ill-conditioned 9-row problem.  The bound is the one the fused route is held to on
    this fixture (tests/test_golden_fixtures.py); it is missed by two decades without the refinement through J."""
    g = np.load(os.path.join(GOLDEN, "cfg1_chain24.npz"))
    rig = make_test_character(24)
    B = g["theta0"].shape[0]
    from oracle import oracle as o

    cons = o.Constraints(g["pos_parent"], g["pos_offset"], g["pos_target"], g["pos_weight"], g["ori_parent"], g["ori_offset"], g["ori_target"], g["ori_weight"])
    pb = _problem(torch_cuda, rig, cons, B)
    out = _solve(torch_cuda, pb, g["theta0"], GnOptions.make(**FIXED))
    assert pb.last_route() == "wave"
    rel = np.linalg.norm(out["theta"] - g["theta_final"], axis=1) / np.linalg.norm(g["theta_final"], axis=1)
    print("rel", rel)
    assert rel.max() <= 5e-5, rel
    assert np.array_equal(out["iterations"], g["iterations"])


WIDENED = []


@pytest.mark.parametrize("seed", range(48))
def test_fuzz(torch_cuda, orc, seed):
    rng = np.random.default_rng(5000 + seed)
    J = int(rng.integers(2, 49))
    rig = random_rig(rng, J, ["chain", "star", "bushy"][seed % 3])
    P = rig.num_params
    Kp, Ko = int(rng.integers(1, 9)), int(rng.integers(0, 6))
    pp = rng.integers(0, J, size=Kp).astype(np.int32)
    op = rng.integers(0, J, size=Ko).astype(np.int32)
    B = 3
    cons, th0, _ = make_problem(rig, pp, op, B, seed=seed, perturb=0.25, random_offsets=True, weights="random")
    full = orc.Constraints(cons.pos_parent, cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_parent, cons.ori_offset,
                           cons.ori_target, cons.ori_weight, pos_function_weight=0.9, ori_function_weight=1.1)  # fmt: skip
    en = (rng.uniform(size=P) < 0.8).astype(np.uint8)
    en[:3] = 1
    en[np.flatnonzero(en)[32:]] = 0  # at most 32 enabled, hence n <= 32
    opt = GnOptions.make(min_iterations=5, max_iterations=5, regularization=0.5, do_line_search=(1 + seed % 2) if seed % 5 == 4 else 0)
    pb = _problem(torch_cuda, rig, cons, B, pos_function_weight=0.9, ori_function_weight=1.1)
    pb.set_enabled(en)
    out = _solve(torch_cuda, pb, th0, opt)
    assert pb.last_route() == "wave"
    ref = orc.solve_batch(rig, full, th0, opt, enabled=en, dtype="f64")
    rel = _rel(out["theta"], ref["theta"])
    tol = np.full(B, 2e-5)
    if np.any(rel > tol):
        ref32 = orc.solve_batch(rig, full, th0, opt, enabled=en, dtype="f32")
        tol = np.maximum(tol, 3.0 * _rel(ref32["theta"], ref["theta"]))
        WIDENED.append(seed)
    print("seed %d J %d P %d n<=%d worst rel %.3e widened seeds so far %s" % (seed, J, P, int(en.sum()), rel.max(), WIDENED))
    assert len(WIDENED) <= 2, WIDENED
    assert np.all(rel <= tol), (seed, rel, tol)
    assert np.array_equal(out["iterations"], ref["iterations"])
    assert np.array_equal(out["status"] & 3, ref["status"])
    h, href = out["error_history"], ref["error_history"]
    assert np.abs(h - href).max() <= 1e-4 * max(1.0, np.abs(href).max())
    assert np.all(out["theta"][:, en == 0] == th0[:, en == 0])


def test_per_instance_rigs(torch_cuda, orc):
    import copy

    rig = make_test_character(24)
    B = 16
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
    rng = np.random.default_rng(77)
    off = (rig.translation_offset[None] * rng.uniform(0.8, 1.2, size=(B, rig.num_joints, 1))).astype(np.float32)
    opt = GnOptions.make(**FIXED)
    pb = _problem(torch_cuda, rig, cons, B)
    pb.set_instance_rig(off, None)
    out = _solve(torch_cuda, pb, th0, opt)
    assert pb.last_route() == "wave"
    for b in range(B):
        rb = copy.deepcopy(rig)
        rb.translation_offset[:] = off[b]
        ref = orc.solve(rb, cons.instance(b), th0[b], opt, dtype="f64")
        rel = np.linalg.norm(out["theta"][b] - ref["theta"]) / max(np.linalg.norm(ref["theta"]), 1e-3)
        assert rel <= 1e-5, (b, rel)
        assert int(out["iterations"][b]) == ref["iterations"] and int(out["status"][b]) & 3 == ref["status"]
        href = np.asarray(ref["error_history"])
        assert np.abs(out["error_history"][b][: len(href)] - href).max() <= 1e-4 * max(1.0, np.abs(href).max())


@pytest.mark.parametrize("case", ["zero_weight_constraint", "function_weight_column_off", "orientation_only", "position_only"])
def test_switched_off_pieces(torch_cuda, orc, case):
    rig = make_test_character(24)
    B = 32
    jj = _all_joints(rig)
    pp, op = jj, jj
    if case == "orientation_only":
        pp = np.zeros(0, np.int32)
    if case == "position_only":
        op = np.zeros(0, np.int32)
    cons, th0, _ = make_problem(rig, pp, op, B, seed=12345, perturb=0.3)
    kw = {}
    fw = None
    if case == "zero_weight_constraint":
        cons.pos_weight[:, 5] = 0.0
        cons.ori_weight[::2, 7] = 0.0
    if case == "function_weight_column_off":
        fw = np.ones((B, 2), np.float32)
        fw[::3, 0] = 0.0  # the position block is off for these elements
        fw[1::4, 1] = 0.0
        fw[2::5, 0] = 0.5
        kw["function_weights"] = fw
    opt = GnOptions.make(**FIXED)
    pb = _problem(torch_cuda, rig, cons, B, **kw)
    out = _solve(torch_cuda, pb, th0, opt)
    assert pb.last_route() == "wave"
    full = orc.Constraints(cons.pos_parent, cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_parent, cons.ori_offset,
                           cons.ori_target, cons.ori_weight, function_weights=fw)  # fmt: skip
    ref = orc.solve_batch(rig, full, th0, opt, dtype="f64")
    _check_fixed(out, ref, th0)


def test_shape_independence(torch_cuda):
    torch = torch_cuda
    rig = make_test_character(24)
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, 64, seed=12345, perturb=0.3)
    opt = GnOptions.make(do_line_search=2, **DRIVER)
    keys = ("theta", "error_history", "iterations", "status")

    def run(B):
        idx = np.arange(B) % 64
        pb = _problem(torch, rig, cons.subset(idx), B)
        out = _solve(torch, pb, th0[idx], opt)
        assert pb.last_route() == "wave"
        return out

    runs = {B: run(B) for B in (1, 3, 64, 4097)}
    again = {B: run(B) for B in (3, 4097)}
    for B in again:
        for k in keys:
            assert np.array_equal(runs[B][k], again[B][k], equal_nan=True), (B, k)
    big = runs[4097]
    for k in keys:
        for B in (1, 3, 64):
            assert np.array_equal(runs[B][k], big[k][:B], equal_nan=True), (B, k)
        tiles = big[k][: 64 * 64].reshape(64, 64, *big[k].shape[1:])
        assert np.all(tiles == tiles[:1]), k
        assert np.array_equal(big[k][4096], big[k][0])


def _expect_unsupported(torch, pb, th0, opt, **kw):
    t = torch.from_numpy(th0.copy()).to(pb.device)
    with pytest.raises(capi.MmxError) as ei:
        pb.solve(t, opt, **kw)
    assert ei.value.code == 4, str(ei.value)  # MMX_ERR_UNSUPPORTED
    assert "MMX_ROUTE_WAVE" in str(ei.value)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), th0)


def test_refusals(torch_cuda):
    torch = torch_cuda
    from momentum_amd._abi import MMX_PRECISION_AUTO, MMX_PRECISION_F64, MMX_PRECISION_MIXED, MMX_STEP_LM_SCHEDULE
    from tests.test_oracle_joint_blocks import make_block

    B = 8
    hum = make_humanoid72(seed=12345, variant="p128", unit=0.01)
    lm = humanoid72_landmark_joints(hum)
    cons, th0, _ = make_problem(hum, lm, lm, B, seed=1, perturb=0.2)
    _expect_unsupported(torch, _problem(torch, hum, cons, B), th0, GnOptions.make(**FIXED))

    rig = make_test_character(24)
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
    opt = GnOptions.make(**FIXED)
    P = rig.num_params
    rng = np.random.default_rng(3)
    plane = make_block(_abi.MMX_JC_PLANE, np.array([3, 9], np.int32), rng, weight=1.0, batch=B)
    cases = {
        "parameter limit": dict(limits=[ParameterLimit.minmax(7, -0.05, 0.05, 1.0)]),
        "model-parameter target": dict(model_target=np.zeros((B, P), np.float32), model_weights=np.ones((B, P), np.float32)),
        "plane block": dict(joint_blocks=[plane]),
        "robust loss": dict(pos_loss=(0.0, 1.0)),
    }
    for name, kw in cases.items():
        pb = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
        f = lambda a, shp: np.ascontiguousarray(a, np.float32).reshape(shp)
        pb.set_constraints(f(cons.pos_offset, (B, cons.Kp, 3)), f(cons.pos_target, (B, cons.Kp, 3)), f(cons.pos_weight, (B, cons.Kp)),
                           f(cons.ori_offset, (B, cons.Ko, 4)), f(cons.ori_target, (B, cons.Ko, 4)), f(cons.ori_weight, (B, cons.Ko)), **kw)  # fmt: skip
        pb.set_route("wave")
        _expect_unsupported(torch, pb, th0, opt)
    pb = _problem(torch, rig, cons, B)
    for kw in (dict(step_rule=MMX_STEP_LM_SCHEDULE), dict(step_rule=_abi.MMX_STEP_TRUST_REGION), dict(precision=MMX_PRECISION_MIXED),
               dict(precision=MMX_PRECISION_AUTO), dict(precision=MMX_PRECISION_F64)):  # fmt: skip
        _expect_unsupported(torch, pb, th0, GnOptions.make(**FIXED, **kw))
    _expect_unsupported(torch, pb, th0, GnOptions.make(step_rule=MMX_STEP_LM_SCHEDULE, **FIXED), want_step_history=True)
    pb.set_instance_parents(np.tile(jj, (B, 1)), np.tile(jj, (B, 1)))
    _expect_unsupported(torch, pb, th0, opt)
    pb.set_instance_parents(None, None)
    out = _solve(torch, pb, th0, opt)  # ... and the handle still solves
    assert pb.last_route() == "wave" and np.all(out["status"] & 3 == 0)
    with pytest.raises(capi.MmxError) as ei:
        pb.solve_diagnostics()
    assert ei.value.code == 4


def test_auto_is_untouched(torch_cuda):
    if os.environ.get("MMX_TEST_ROUTE"):
        pytest.skip("a MMX_TEST_ROUTE sweep pins the route")
    torch = torch_cuda
    rig = make_test_character(24)
    B = 64
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
    opt = GnOptions.make(**FIXED)
    pa = _problem(torch, rig, cons, B, route="auto")
    oa = _solve(torch, pa, th0, opt)
    assert pa.last_route() == "fused"
    pf = _problem(torch, rig, cons, B, route="fused")
    of = _solve(torch, pf, th0, opt)
    for k in ("theta", "error", "iterations", "status", "error_history"):
        assert np.array_equal(oa[k], of[k]), k


def test_graph_capture(torch_cuda):
    torch = torch_cuda
    rig = make_test_character(24)
    B = 128
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
    pb = _problem(torch, rig, cons, B)
    opt = GnOptions.make(do_line_search=2, **DRIVER)
    dev = pb.device
    outs = lambda: dict(error=torch.empty((B,), dtype=torch.float64, device=dev), iterations=torch.empty((B,), dtype=torch.int32, device=dev),
                        status=torch.empty((B,), dtype=torch.int32, device=dev), error_history=torch.empty((B, 50), dtype=torch.float64, device=dev))  # fmt: skip
    o = outs()
    t = torch.from_numpy(th0.copy()).to(dev)
    pb.solve(t, opt, outputs=o)
    torch.cuda.synchronize()
    assert pb.last_route() == "wave"
    ref = {k: v.cpu().numpy() for k, v in o.items()}
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
    for _ in range(2):
        for v in go.values():
            if v is not theta:
                v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in ("theta", "error", "iterations", "status", "error_history"):
            assert np.array_equal(go[k].cpu().numpy(), ref[k]), k


def test_non_finite_input(torch_cuda):
    torch = torch_cuda
    rig = make_test_character(24)
    B = 8
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
    opt = GnOptions.make(**FIXED)
    sound = _solve(torch, _problem(torch, rig, cons, B), th0, opt)
    cons.pos_target[2, 4, 1] = np.nan
    pb = _problem(torch, rig, cons, B)
    out = _solve(torch, pb, th0, opt)
    assert pb.last_route() == "wave"
    assert out["status"][2] & 3 != 0
    assert np.array_equal(out["theta"][2], th0[2])
    keep = np.arange(B) != 2
    for k in ("theta", "error", "iterations", "status", "error_history"):
        assert np.array_equal(out[k][keep], sound[k][keep]), k


def test_solver2_surface(torch_cuda, orc):
    from momentum_amd import solver2 as s2

    rig = make_test_character(3)
    B = 32
    jj = _all_joints(rig)
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
    ch = s2.Character(rig)
    pe = s2.PositionErrorFunction(ch)
    oe = s2.OrientationErrorFunction(ch)
    pe.add_constraints(jj, cons.pos_target, cons.pos_offset, cons.pos_weight)
    oe.add_constraints(cons.ori_target, jj, cons.ori_offset, cons.ori_weight)
    fn = s2.SkeletonSolverFunction(ch, [pe, oe])
    so = s2.GaussNewtonSolverQROptions()
    so.min_iterations, so.max_iterations, so.threshold, so.regularization, so.do_line_search = 4, 50, 10.0, 0.01, True
    solver = s2.GaussNewtonSolverQR(fn, so)
    assert solver.set_route("wave") is solver
    th = solver.solve(th0)
    assert fn._cache[1].last_route() == "wave"
    opt = GnOptions.make(do_line_search=2, **DRIVER)
    ref = orc.solve_batch(rig, cons, th0, opt, dtype="f64")
    rel = _rel(th, ref["theta"])
    assert np.all(rel <= 1e-5), rel.max()
    assert np.array_equal(np.zeros(B, np.int32), ref["status"])
    direct = _solve(torch_cuda, _problem(torch_cuda, rig, cons, B), th0, opt)
    hist = solver.per_iteration_errors
    assert [len(h) for h in hist] == [int(i) for i in direct["iterations"]]
    assert all(4 <= len(h) <= 50 for h in hist)
    assert np.abs(direct["error"] - ref["error"]).max() <= 1e-4 * max(1.0, np.abs(ref["error"]).max())
