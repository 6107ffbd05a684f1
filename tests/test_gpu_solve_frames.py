"""mmx_solve_frames: warm-started frame sequences in one launch (waveSolveKernel<NP, true>: momentum_amd/csrc/mmx_wave.hip,
built as mmx_wave_frames.hip).

The batch is F x S instances, frame-major; frame f of sequence s must be solved exactly as `solve` on the pinned "wave" route
solves instance f S + s, started from the result row of frame f - 1.  The exact reference is therefore a CHAIN of F whole-batch
`solve` calls on the same handle (the route's results do not depend on batch size or position, tests/test_gpu_wave_route.py
test_shape_independence): before call f the rows of frame f are set to call f - 1's rows of frame f - 1 (f = 0: the caller's),
and frame f's rows of every output are taken from call f.  Equality is np.array_equal on everything.

Against the oracle's DOUBLE run, chained frame by frame on the CPU: rel = |theta - theta_f64| / max(|theta_f64|, 1e-3) <= 1e-5
on every frame of every sequence (the oracle's own float chain on these inputs stays at or below 6.4e-6)."""
import os

import numpy as np
import pytest

from momentum_amd import _abi, capi, make_humanoid72, humanoid72_landmark_joints, make_test_character
from momentum_amd._abi import GnOptions, ParameterLimit
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu
FIXED = dict(min_iterations=10, max_iterations=10, threshold=1.0, regularization=0.05)
DRIVER = dict(min_iterations=4, max_iterations=50, threshold=10.0, regularization=0.01)
OPTIONS = {
    "fixed": dict(FIXED),
    "driver": dict(do_line_search=0, **DRIVER),
    "driver_ls1": dict(do_line_search=1, **DRIVER),
    "driver_ls2": dict(do_line_search=2, **DRIVER),
}
KEYS = ("theta", "error", "iterations", "status", "error_history", "parameter_history")
_CACHE = {}


def _inputs(name, count, **kw):
    """(rig, constraints [count, ...], theta0 [count, P]) of make_problem on every joint, computed once and left unchanged."""
    key = (name, count, tuple(sorted(kw.items())))
    if key not in _CACHE:
        rig = make_test_character(3 if name == "char3" else 24)
        jj = np.arange(rig.num_joints, dtype=np.int32)
        cons, th0, _ = make_problem(rig, jj, jj, count, seed=12345, perturb=0.3, **kw)
        _CACHE[key] = (rig, cons, th0)
    return _CACHE[key]


def _problem(torch, rig, cons, B, route="wave", **kw):
    pb = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
    t = lambda a, shp: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shp)).to(pb.device)
    if kw.get("function_weights") is not None:
        kw["function_weights"] = t(kw["function_weights"], np.asarray(kw["function_weights"]).shape)
    pb.set_constraints(t(cons.pos_offset, (B, cons.Kp, 3)), t(cons.pos_target, (B, cons.Kp, 3)), t(cons.pos_weight, (B, cons.Kp)),
                       t(cons.ori_offset, (B, cons.Ko, 4)), t(cons.ori_target, (B, cons.Ko, 4)), t(cons.ori_weight, (B, cons.Ko)), **kw)  # fmt: skip
    pb.set_route(route)
    return pb


def _host(torch, out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _chain(torch, pb, init, opt, F):
    """The reference: F whole-batch solves, frame f's rows seeded from call f - 1's frame f - 1 rows, taken from call f."""
    S, P = init.shape
    B = F * S
    theta = np.full((B, P), 0.25, np.float32)  # (the other rows may hold anything)
    prev = init
    ref = None
    for f in range(F):
        rows = slice(f * S, (f + 1) * S)
        theta[rows] = prev
        out = _host(torch, pb.solve(torch.from_numpy(theta.copy()).to(pb.device), opt, want_history=True, want_parameter_history=True))
        assert pb.last_route() == "wave"
        if ref is None:
            ref = {k: np.zeros_like(out[k]) for k in KEYS}
        for k in KEYS:
            ref[k][rows] = out[k][rows]
        prev = out["theta"][rows]
        theta = out["theta"]
    return ref


def _frames(torch, pb, init, opt, F, rest=0.0, shape3=False):
    S, P = init.shape
    theta = np.full((F * S, P), rest, np.float32)  # the rows of frames >= 1 are not read
    theta[:S] = init
    t = torch.from_numpy(theta.reshape(F, S, P) if shape3 else theta).to(pb.device)
    out = _host(torch, pb.solve_frames(t, opt, F, want_history=True, want_parameter_history=True))
    assert pb.last_route() == "wave"
    out["theta"] = out["theta"].reshape(F * S, P)
    return out


def _assert_equal(out, ref, tag=""):
    for k in KEYS:
        assert np.array_equal(out[k], ref[k], equal_nan=True), (tag, k)


@pytest.mark.parametrize("S", [1, 3, 4, 5])
@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("name", ["char3", "chain24"])
def test_equals_chained_solves(torch_cuda, name, options, S):
    """16-column (3-joint character) and 32-column (24-joint chain) instantiations; S around the four waves of a workgroup;
    the line-search cases are the ones that joint states left in LDS by the previous frame's last trial would break."""
    rig, cons_all, th_all = _inputs(name, 35)
    opt = GnOptions.make(**OPTIONS[options])
    for F in (1, 2, 7):
        B = F * S
        idx = np.arange(B)
        pb = _problem(torch_cuda, rig, cons_all.subset(idx), B)
        init = th_all[:S] + np.float32(0.05)
        ref = _chain(torch_cuda, pb, init, opt, F)
        out = _frames(torch_cuda, pb, init, opt, F, shape3=(F == 2))
        _assert_equal(out, ref, (name, options, S, F))
        assert np.all(out["status"] & 3 == 0)


def test_one_frame_is_plain_solve(torch_cuda):
    rig, cons_all, th_all = _inputs("chain24", 35)
    B = 5
    opt = GnOptions.make(**OPTIONS["driver_ls2"])
    pb = _problem(torch_cuda, rig, cons_all.subset(np.arange(B)), B, route="auto")
    out = _frames(torch_cuda, pb, th_all[:B], opt, 1)  # (MMX_ROUTE_AUTO is accepted, and the wave route is what ran)
    plain = _host(torch_cuda, pb.solve(torch_cuda.from_numpy(th_all[:B].copy()).to(pb.device), opt, want_history=True, want_parameter_history=True))
    if not os.environ.get("MMX_TEST_ROUTE"):  # (a sweep pins the route of `solve`)
        assert pb.last_route() == "fused"  # mmx_solve's own routing is unchanged: AUTO never picks the wave route there
    pb.set_route("wave")
    plain = _host(torch_cuda, pb.solve(torch_cuda.from_numpy(th_all[:B].copy()).to(pb.device), opt, want_history=True, want_parameter_history=True))
    _assert_equal(out, plain)


def test_later_input_rows_are_not_read(torch_cuda):
    rig, cons_all, th_all = _inputs("chain24", 35)
    S, F = 3, 4
    opt = GnOptions.make(**OPTIONS["driver_ls2"])
    pb = _problem(torch_cuda, rig, cons_all.subset(np.arange(F * S)), F * S)
    ref = _chain(torch_cuda, pb, th_all[:S], opt, F)
    out = _frames(torch_cuda, pb, th_all[:S], opt, F, rest=np.nan)
    _assert_equal(out, ref)
    assert np.all(np.isfinite(out["theta"])) and np.all(out["status"] & 3 == 0)


@pytest.mark.parametrize("variant", ["enabled_mask", "instance_rigs", "function_weights"])
def test_variants(torch_cuda, variant):
    rig, cons_all, th_all = _inputs("chain24", 35)
    S, F = 3, 4
    B = F * S
    opt = GnOptions.make(**OPTIONS["driver_ls2"])
    rng = np.random.default_rng(99)
    kw = {}
    if variant == "function_weights":
        kw["function_weights"] = rng.uniform(0.3, 1.7, size=(B, 2)).astype(np.float32)
    pb = _problem(torch_cuda, rig, cons_all.subset(np.arange(B)), B, **kw)
    en = None
    if variant == "enabled_mask":
        en = (rng.uniform(size=rig.num_params) < 0.7).astype(np.uint8)
        en[:3] = 1
        pb.set_enabled(en)
    if variant == "instance_rigs":
        off = (rig.translation_offset[None] * rng.uniform(0.8, 1.2, size=(B, rig.num_joints, 1))).astype(np.float32)
        pb.set_instance_rig(off, None)
    init = th_all[:S] + np.float32(0.05)
    ref = _chain(torch_cuda, pb, init, opt, F)
    out = _frames(torch_cuda, pb, init, opt, F, rest=np.nan)
    _assert_equal(out, ref, variant)
    if en is not None:  # disabled parameters carry frame 0's values through every row
        got = out["theta"].reshape(F, S, -1)
        assert np.array_equal(got[:, :, en == 0], np.broadcast_to(init[None][:, :, en == 0], (F, S, int((en == 0).sum()))))
    if variant != "enabled_mask":  # the variant's payload is indexed by instance: a frame's differs from its neighbour's
        assert not np.array_equal(out["error"][:S], out["error"][S : 2 * S])


@pytest.mark.parametrize("options", ["fixed", "driver_ls2"])
@pytest.mark.parametrize("name,kw", [("char3", {}), ("chain24", {}), ("char3", dict(random_offsets=True, weights="random")),
                                     ("chain24", dict(random_offsets=True, weights="random"))])  # fmt: skip
def test_against_double_oracle_chain(torch_cuda, orc, name, kw, options):
    rig, cons, th0 = _inputs(name, 30, **kw)
    F, S = 6, 5
    opt = GnOptions.make(**OPTIONS[options])
    pb = _problem(torch_cuda, rig, cons, F * S)
    out = _frames(torch_cuda, pb, th0[:S], opt, F)
    prev = th0[:S].astype(np.float64)
    worst = []
    for f in range(F):
        rows = np.arange(f * S, (f + 1) * S)
        ref = orc.solve_batch(rig, cons.subset(rows), prev, opt, dtype="f64")
        th = out["theta"][rows]
        rel = np.linalg.norm(th - ref["theta"], axis=1) / np.maximum(np.linalg.norm(ref["theta"], axis=1), 1e-3)
        worst.append(float(rel.max()))
        print("frame %d worst rel %.3e" % (f, rel.max()))
        assert np.all(rel <= 1e-5), (f, rel)
        if options == "fixed":
            assert np.array_equal(out["iterations"][rows], ref["iterations"])
            assert np.array_equal(out["status"][rows] & 3, ref["status"])
        else:
            assert np.all((out["iterations"][rows] >= 4) & (out["iterations"][rows] <= 50))
        prev = ref["theta"]
    print("worst rel per frame", worst)


def test_non_finite_frame(torch_cuda):
    rig, cons_all, th_all = _inputs("chain24", 35)
    S, F = 3, 5
    B = F * S
    cons = cons_all.subset(np.arange(B))  # (a copy: the shared inputs stay as they are)
    bad = 2 * S + 1  # frame 2 of sequence 1
    cons.pos_target.reshape(B, cons.Kp, 3)[bad, 4, 1] = np.nan
    opt = GnOptions.make(**FIXED)
    pb = _problem(torch_cuda, rig, cons, B)
    ref = _chain(torch_cuda, pb, th_all[:S], opt, F)
    out = _frames(torch_cuda, pb, th_all[:S], opt, F)
    assert out["status"][bad] & 3 != 0
    assert np.array_equal(out["theta"][bad], out["theta"][bad - S])  # its own initial parameters: frame 1's result row
    assert np.all(np.isfinite(out["theta"]))
    keep = np.arange(B) != bad
    assert np.all(out["status"][keep] & 3 == 0)
    _assert_equal(out, ref)
    # sequences 0 and 2 never met the NaN: they equal the chain on the sound payload
    sound = _chain(torch_cuda, _problem(torch_cuda, rig, cons_all.subset(np.arange(B)), B), th_all[:S], opt, F)
    others = np.arange(B) % S != 1
    for k in KEYS:
        assert np.array_equal(out[k][others], sound[k][others]), k
    before = np.arange(B) < bad  # ... and sequence 1 up to the frame before
    for k in KEYS:
        assert np.array_equal(out[k][before], sound[k][before]), k


def test_graph_capture(torch_cuda):
    torch = torch_cuda
    rig, cons_all, th_all = _inputs("chain24", 35)
    S, F = 8, 4
    B = S * F
    pb = _problem(torch, rig, cons_all.subset(np.arange(B)), B)
    opt = GnOptions.make(**OPTIONS["driver_ls2"])
    dev = pb.device
    outs = lambda: dict(error=torch.empty((B,), dtype=torch.float64, device=dev), iterations=torch.empty((B,), dtype=torch.int32, device=dev),
                        status=torch.empty((B,), dtype=torch.int32, device=dev), error_history=torch.empty((B, 50), dtype=torch.float64, device=dev))  # fmt: skip
    th0 = np.zeros((B, rig.num_params), np.float32)
    th0[:S] = th_all[:S]
    o = outs()
    pb.solve_frames(torch.from_numpy(th0.copy()).to(dev), opt, F, outputs=o)  # warm-up = the eager call
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
            pb.solve_frames(theta, opt, F, outputs=go)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for v in go.values():
            if v is not theta:
                v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in ("theta", "error", "iterations", "status", "error_history"):
            assert np.array_equal(go[k].cpu().numpy(), ref[k]), k


def _expect_refusal(torch, pb, th0, opt, F, code, names_route=True):
    t = torch.from_numpy(th0.copy()).to(pb.device)
    with pytest.raises(capi.MmxError) as ei:
        pb.solve_frames(t, opt, F)
    assert ei.value.code == code, str(ei.value)
    if names_route:
        assert "MMX_ROUTE_WAVE" in str(ei.value)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), th0)


def test_refusals(torch_cuda):
    torch = torch_cuda
    B = 12
    hum = make_humanoid72(seed=12345, variant="p128", unit=0.01)
    lm = humanoid72_landmark_joints(hum)
    cons, th0, _ = make_problem(hum, lm, lm, B, seed=1, perturb=0.2)
    _expect_refusal(torch, _problem(torch, hum, cons, B), th0, GnOptions.make(**FIXED), 3, 4)

    rig, cons_all, th_all = _inputs("chain24", 35)
    cons, th0 = cons_all.subset(np.arange(B)), th_all[:B]
    opt = GnOptions.make(**FIXED)
    pb = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
    f = lambda a, shp: np.ascontiguousarray(a, np.float32).reshape(shp)
    pb.set_constraints(f(cons.pos_offset, (B, cons.Kp, 3)), f(cons.pos_target, (B, cons.Kp, 3)), f(cons.pos_weight, (B, cons.Kp)),
                       f(cons.ori_offset, (B, cons.Ko, 4)), f(cons.ori_target, (B, cons.Ko, 4)), f(cons.ori_weight, (B, cons.Ko)),
                       limits=[ParameterLimit.minmax(7, -0.05, 0.05, 1.0)])  # fmt: skip
    pb.set_route("wave")
    _expect_refusal(torch, pb, th0, opt, 3, 4)

    pb = _problem(torch, rig, cons, B)
    _expect_refusal(torch, pb, th0, opt, 0, 1, names_route=False)  # MMX_ERR_INVALID_ARGUMENT
    _expect_refusal(torch, pb, th0, opt, 5, 1, names_route=False)  # 12 is no multiple of 5
    _expect_refusal(torch, pb, th0, GnOptions.make(step_rule=_abi.MMX_STEP_LM_SCHEDULE, **FIXED), 3, 4)
    _expect_refusal(torch, pb, th0, GnOptions.make(precision=_abi.MMX_PRECISION_MIXED, **FIXED), 3, 4)
    pb.set_route("fused")
    _expect_refusal(torch, pb, th0, opt, 3, 4, names_route=False)
    pb.set_route("wave")  # ... and the handle still solves
    S, F = 4, 3
    ref = _chain(torch, pb, th0[:S], opt, F)
    out = _frames(torch, pb, th0[:S], opt, F)
    _assert_equal(out, ref)
    assert np.all(out["status"] & 3 == 0)


def test_solver2_surface(torch_cuda):
    from momentum_amd import solver2 as s2

    rig, cons_all, th_all = _inputs("char3", 35)
    S, F = 3, 4
    B = S * F
    cons = cons_all.subset(np.arange(B))
    jj = np.arange(rig.num_joints, dtype=np.int32)
    ch = s2.Character(rig)
    pe = s2.PositionErrorFunction(ch)
    oe = s2.OrientationErrorFunction(ch)
    pe.add_constraints(jj, cons.pos_target, cons.pos_offset, cons.pos_weight)
    oe.add_constraints(cons.ori_target, jj, cons.ori_offset, cons.ori_weight)
    fn = s2.SkeletonSolverFunction(ch, [pe, oe])
    so = s2.GaussNewtonSolverQROptions()
    so.min_iterations, so.max_iterations, so.threshold, so.regularization, so.do_line_search = 4, 50, 10.0, 0.01, True
    solver = s2.GaussNewtonSolverQR(fn, so).set_route("wave")
    th0 = np.zeros((B, rig.num_params), np.float32)
    th0[:S] = th_all[:S]
    th = solver.solve_frames(th0, F)
    assert fn._cache[1].last_route() == "wave"
    direct = _frames(torch_cuda, _problem(torch_cuda, rig, cons, B), th_all[:S], GnOptions.make(**OPTIONS["driver_ls2"]), F)
    assert np.array_equal(th, direct["theta"])
    assert [len(h) for h in solver.per_iteration_errors] == [int(i) for i in direct["iterations"]]
    th3 = solver.solve_frames(th0.reshape(F, S, -1), F)
    assert th3.shape == (F, S, rig.num_params) and np.array_equal(th3.reshape(B, -1), direct["theta"])
