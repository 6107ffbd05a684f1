"""mmx_eval_gradient (Problem.eval_gradient): the batched error and gradient 2 J^T r without a Jacobian, against the CPU oracle.

Reference, per instance: oracle.eval_jacobian(rig, cons.instance(b), theta, enabled, "f64") gives g64 = 2 J^T r in double and
e64.  The bound is computed from the reference itself, not guessed: g32 / e32 are the same quantities from the oracle's own
"f32" evaluation (the contraction summed in float32), and

    max|g - g64| <= 4 max(max|g32 - g64|, 2.5e-7 max|g64|)        |e - e64| <= 4 max(|e32 - e64|, 2.5e-7 e64)

(4: the summation order differs, subtree sums instead of row order; the floor: an instance where the float oracle happens to
round well must not set an unreachable bound).  The bound sits near 1e-6 .. 4e-6 of max|g64| / e64 on these inputs, which are
away from the minimum.

Deviations the MI355X reaches: per case the instance that comes closest to its bound, relative to max|g64| / e64, the bound in
brackets (measured once with this file's inputs; the worst case uses 0.29 of its gradient bound, 0.25 of its error bound):
  chain24                    gradient 2.83e-07 (1.12e-06)   error 3.44e-07 (1.46e-06)
  chain24_parameter_rows     gradient 2.34e-07 (1.00e-06)   error 1.13e-07 (1.00e-06)
  chain24_third_disabled     gradient 2.83e-07 (1.12e-06)   error 3.44e-07 (1.46e-06)
  chain24_welsch             gradient 2.71e-07 (1.00e-06)   error 8.44e-08 (1.00e-06)
  char3                      gradient 2.28e-07 (1.00e-06)   error 1.23e-07 (1.00e-06)
  char3_instance_rig         gradient 2.95e-07 (1.00e-06)   error 1.29e-07 (1.00e-06)
  char3_l1_cauchy            gradient 1.77e-07 (1.00e-06)   error 3.25e-07 (1.32e-06)
  char3_single               gradient 1.38e-07 (1.00e-06)   error 1.23e-07 (1.00e-06)
  humanoid72                 gradient 3.17e-07 (1.59e-06)   error 7.82e-08 (1.01e-06)
"""
import copy
import functools

import numpy as np
import pytest

from momentum_amd import _abi, capi, humanoid72_landmark_joints, make_humanoid72, make_test_character
from momentum_amd._abi import MMX_LOSS_WELSCH, EllipsoidLimit, JointBlock, ParameterLimit
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu
MMX_ERR_INVALID_ARGUMENT, MMX_ERR_UNSUPPORTED = 1, 4


# ---------------------------------------------------------------------------------------------------------------------
# cases: the smallest shapes at which the kernel can still go wrong
# ---------------------------------------------------------------------------------------------------------------------
def _rig(which):
    if which == "char3":  # P = 10, one tree-sum tile
        rig = make_test_character(3)
        return rig, [0, 1, 2], [1, 2]
    if which == "chain24":  # P = 31, sources shared along a deep chain, constraints on every joint
        rig = make_test_character(24)
        return rig, list(range(24)), list(range(24))
    rig = make_humanoid72(seed=12345, variant="p128")  # five 16-row tiles, dead joints, P = 128
    lm = humanoid72_landmark_joints(rig)
    return rig, lm, lm


def _with(cons, orc, **kw):
    base = dict(limits=cons.limits, limit_function_weight=cons.limit_function_weight, model_target=cons.model_target, model_weights=cons.model_weights,
                model_function_weight=cons.model_function_weight, pos_loss=cons.pos_loss, ori_loss=cons.ori_loss, joint_blocks=cons.joint_blocks,
                ellipsoid_limits=cons.ellipsoid_limits, function_weights=cons.function_weights)  # fmt: skip
    base.update(kw)
    return orc.Constraints(cons.pos_parent, cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_parent, cons.ori_offset, cons.ori_target,
                           cons.ori_weight, **base)  # fmt: skip


CASES = {
    # name: (rig, B, variation)
    "char3": ("char3", 5, None),
    "chain24": ("chain24", 5, None),
    "humanoid72": ("humanoid72", 3, None),
    "char3_single": ("char3", 1, None),
    "chain24_third_disabled": ("chain24", 5, "mask"),
    "char3_l1_cauchy": ("char3", 5, "robust"),
    "chain24_welsch": ("chain24", 3, "welsch"),
    "chain24_parameter_rows": ("chain24", 5, "rows"),
    "char3_instance_rig": ("char3", 5, "instance_rig"),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """dict(rig, rigs (per instance), cons, theta [B,P], enabled or None, offsets or None) of a case; built once."""
    from oracle import oracle as orc

    which, B, var = CASES[name]
    rig, pp, op = _rig(which)
    cons, th0, _ = make_problem(rig, pp, op, B, seed=12345, perturb=0.3, random_offsets=True, weights="random", theta0_scale=0.2)
    P = rig.num_params
    c = dict(rig=rig, rigs=[rig] * B, cons=cons, theta=th0, enabled=None, offsets=None, B=B)
    rng = np.random.default_rng(99)
    if var == "mask":
        en = np.ones(P, np.uint8)
        en[1::3] = 0  # a third of the parameters off
        c["enabled"] = en
    elif var == "robust":
        c["cons"] = _with(cons, orc, pos_loss=(1.0, 0.5), ori_loss=(0.0, 1.0))
    elif var == "welsch":
        c["cons"] = _with(cons, orc, pos_loss=(MMX_LOSS_WELSCH, 1.5), ori_loss=(MMX_LOSS_WELSCH, 1.0))
    elif var == "rows":
        limits = [
            ParameterLimit.minmax(3, -10.0, -5.0, 1.3),  # violated at every theta here (|theta| <= 0.2)
            ParameterLimit.minmax(5, -10.0, 10.0, 0.8),  # never violated
            ParameterLimit.linear(7, 9, 0.7, 0.05, weight=1.1),
        ]
        fw = rng.uniform(0.5, 1.5, size=(B, 4)).astype(np.float32)
        fw[1, 2] = 0.0  # element 1: the limit block off
        c["cons"] = _with(cons, orc, limits=limits, limit_function_weight=0.6, model_target=rng.uniform(-0.2, 0.2, size=(B, P)).astype(np.float32),
                          model_weights=rng.uniform(-0.3, 1.5, size=(B, P)).astype(np.float32), model_function_weight=1.4, function_weights=fw)  # fmt: skip
    elif var == "instance_rig":
        off = np.repeat(rig.translation_offset[None], B, axis=0).astype(np.float32)
        off *= (1.0 + 0.25 * rng.uniform(-1, 1, size=(B, rig.num_joints, 1))).astype(np.float32)
        rigs = []
        for b in range(B):
            r = copy.copy(rig)
            r.translation_offset = np.ascontiguousarray(off[b])
            rigs.append(r)
        c["rigs"], c["offsets"] = rigs, off
    return c


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(g64 [B,P], e64 [B], g32 [B,P], e32 [B]) of a case from the oracle; computed once, never modified."""
    return _reference_of(_case(name))


def _reference_of(c):
    """The same of a case dict (tests/test_gpu_eval_gradient_shapes.py builds its own cases)."""
    from oracle import oracle as orc

    orc.build()
    B, P = c["B"], c["rig"].num_params
    g64, g32, e64, e32 = np.zeros((B, P)), np.zeros((B, P), np.float32), np.zeros(B), np.zeros(B)
    for b in range(B):
        ci = c["cons"].instance(b)
        J, r, e = orc.eval_jacobian(c["rigs"][b], ci, c["theta"][b].astype(np.float64), c["enabled"], "f64")
        g64[b], e64[b] = 2.0 * (J.T @ r), e
        Jf, rf, ef = orc.eval_jacobian(c["rigs"][b], ci, c["theta"][b], c["enabled"], "f32")
        assert Jf.dtype == np.float32 and rf.dtype == np.float32
        g32[b], e32[b] = np.float32(2.0) * (np.ascontiguousarray(Jf.T) @ rf), ef
    for a in (g64, g32, e64, e32):
        a.setflags(write=False)
    return g64, e64, g32, e32


def _problem(c, B=None, cons=None):
    cons = c["cons"] if cons is None else cons
    B = c["B"] if B is None else B
    pb = capi.Problem(capi.RigHandle(c["rig"], 0), B, cons.pos_parent, cons.ori_parent)
    sh = lambda a, *s: np.ascontiguousarray(a, np.float32).reshape(s)
    P = c["rig"].num_params
    pb.set_constraints(
        sh(cons.pos_offset, B, cons.Kp, 3), sh(cons.pos_target, B, cons.Kp, 3), sh(cons.pos_weight, B, cons.Kp),
        sh(cons.ori_offset, B, cons.Ko, 4), sh(cons.ori_target, B, cons.Ko, 4), sh(cons.ori_weight, B, cons.Ko),
        cons.pos_function_weight, cons.ori_function_weight, limits=cons.limits, limit_function_weight=cons.limit_function_weight,
        model_target=None if cons.model_target is None else sh(cons.model_target, B, P),
        model_weights=None if cons.model_weights is None else sh(cons.model_weights, B, P), model_function_weight=cons.model_function_weight,
        pos_loss=cons.pos_loss, ori_loss=cons.ori_loss, joint_blocks=cons.joint_blocks, ellipsoid_limits=cons.ellipsoid_limits,
        function_weights=cons.function_weights,
    )  # fmt: skip
    if c["enabled"] is not None:
        pb.set_enabled(c["enabled"])
    if c["offsets"] is not None:
        pb.set_instance_rig(translation_offset=c["offsets"])
    return pb


def _check(tag, g, e, ref):
    """Prints every figure, then asserts the bound of the module docstring instance by instance."""
    g64, e64, g32, e32 = ref
    bad = []
    for b in range(g64.shape[0]):
        gs = np.abs(g64[b]).max()
        dg, bg = np.abs(g[b].astype(np.float64) - g64[b]).max(), 4.0 * max(np.abs(g32[b].astype(np.float64) - g64[b]).max(), 2.5e-7 * gs)
        de, be = abs(e[b] - e64[b]), 4.0 * max(abs(e32[b] - e64[b]), 2.5e-7 * e64[b])
        print(f"{tag} b={b}: max|g64| {gs:.4g} gradient {dg / gs:.3g} (bound {bg / gs:.3g}) error {de / e64[b]:.3g} (bound {be / e64[b]:.3g})")
        assert gs > 1.0 and e64[b] > 0.0  # away from the minimum: the relative bound means something
        if not (dg <= bg and de <= be):
            bad.append((b, dg / gs, bg / gs, de / e64[b], be / e64[b]))
    assert not bad, (tag, bad)


def _eval(torch, pb, theta, **kw):
    g, e = pb.eval_gradient(torch.from_numpy(np.ascontiguousarray(theta, np.float32)).to(pb.device), **kw)
    torch.cuda.synchronize()
    return None if g is None else g.cpu().numpy(), None if e is None else e.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_and_error_hold_the_oracle_bound(torch_cuda, name):
    torch = torch_cuda
    c = _case(name)
    pb = _problem(c)
    g, e = _eval(torch, pb, c["theta"])
    assert g.shape == (c["B"], c["rig"].num_params) and g.dtype == np.float32 and e.dtype == np.float64
    _check(name, g, e, _reference(name))
    g64 = _reference(name)[0]
    if c["enabled"] is not None:
        off = c["enabled"] == 0
        assert off.sum() >= c["rig"].num_params // 3 and np.all(g[:, off] == 0.0)  # exact zeros, sign included
        assert not np.signbit(g[:, off]).any()
    assert np.all(g[g64 == 0.0] == 0.0)  # structurally zero columns (and rows of switched-off blocks) too


@pytest.mark.parametrize("name", ["char3", "chain24_parameter_rows", "humanoid72"])
def test_gradient_matches_the_handles_own_jacobian(torch_cuda, name):
    """2 J^T r of mmx_eval_jacobian's own J and r, contracted in float64 on the host, in place of g64 / e64: the two entry
    points of one library under the same bound."""
    torch = torch_cuda
    c = _case(name)
    pb = _problem(c)
    jac, res, err = pb.eval_jacobian(torch.from_numpy(c["theta"]).to(pb.device))
    J, r = jac.cpu().numpy().astype(np.float64).transpose(0, 2, 1), res.cpu().numpy().astype(np.float64)
    gj = 2.0 * np.einsum("bmp,bm->bp", J, r)
    g, e = _eval(torch, pb, c["theta"])
    _, _, g32, e32 = _reference(name)
    g64, e64 = _reference(name)[:2]
    # (the oracle's float deviation measured against its own double evaluation sets the bound; the Jacobian's values stand
    # where g64 / e64 stood)
    ref = (gj, err.cpu().numpy(), gj + (g32.astype(np.float64) - g64), err.cpu().numpy() + (e32 - e64))
    _check(name + " vs eval_jacobian", g, e, ref)


def test_forms_are_bitwise_the_same_outputs_and_neither_is_refused(torch_cuda):
    torch = torch_cuda
    for name in ("chain24_parameter_rows", "humanoid72"):
        c = _case(name)
        pb = _problem(c)
        g, e = _eval(torch, pb, c["theta"])
        g_only, none_e = _eval(torch, pb, c["theta"], want_err=False)
        none_g, e_only = _eval(torch, pb, c["theta"], want_grad=False)
        assert none_e is None and none_g is None
        assert np.array_equal(g_only, g) and np.array_equal(e_only, e)
        with pytest.raises(capi.MmxError) as ei:
            pb.eval_gradient(torch.from_numpy(c["theta"]).to(pb.device), want_grad=False, want_err=False)
        assert ei.value.code == MMX_ERR_INVALID_ARGUMENT


def test_rows_do_not_depend_on_batch_position_or_run(torch_cuda):
    torch = torch_cuda
    c = _case("chain24_parameter_rows")
    cons, B, P = c["cons"], c["B"], c["rig"].num_params
    alone = _eval(torch, _problem(c), c["theta"])
    # the same five instances at positions 9, 2, 30, 17, 36 of a batch of 37, other instances around them
    where, BB = [9, 2, 30, 17, 36], 37
    rig, pp, op = _rig("chain24")
    big, thb, _ = make_problem(rig, pp, op, BB, seed=777, perturb=0.3, random_offsets=True, weights="random", theta0_scale=0.2)
    rng = np.random.default_rng(5)
    mt, mw = rng.uniform(-0.2, 0.2, size=(BB, P)).astype(np.float32), rng.uniform(-0.3, 1.5, size=(BB, P)).astype(np.float32)
    fw = rng.uniform(0.5, 1.5, size=(BB, 4)).astype(np.float32)
    arrays = dict(pos_offset=big.pos_offset.copy(), pos_target=big.pos_target.copy(), pos_weight=big.pos_weight.copy(), ori_offset=big.ori_offset.copy(),
                  ori_target=big.ori_target.copy(), ori_weight=big.ori_weight.copy(), model_target=mt, model_weights=mw, function_weights=fw)  # fmt: skip
    theta = thb.copy()
    for b, w in enumerate(where):
        for k, a in arrays.items():
            a[w] = getattr(cons, k).reshape((B,) + a.shape[1:])[b]
        theta[w] = c["theta"][b]
    from oracle import oracle as orc

    big = orc.Constraints(big.pos_parent, arrays["pos_offset"], arrays["pos_target"], arrays["pos_weight"], big.ori_parent, arrays["ori_offset"],
                          arrays["ori_target"], arrays["ori_weight"], limits=cons.limits, limit_function_weight=cons.limit_function_weight,
                          model_target=mt, model_weights=mw, model_function_weight=cons.model_function_weight, function_weights=fw)  # fmt: skip
    pbb = _problem(c, BB, big)
    first = _eval(torch, pbb, theta)
    second = _eval(torch, pbb, theta)
    for got in (first, second):
        assert np.array_equal(got[0][where], alone[0]) and np.array_equal(got[1][where], alone[1])
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_problems_outside_the_scope_are_refused_before_any_output_is_touched(torch_cuda):
    torch = torch_cuda
    from oracle import oracle as orc

    c = _case("char3")
    B, rig = c["B"], c["rig"]
    rng = np.random.default_rng(17)
    K = 2
    plane = JointBlock(_abi.MMX_JC_PLANE, [1, 2], np.full((B, K), 2.0, np.float32), rng.uniform(0.1, 1, (B, K, 3)).astype(np.float32),
                       local_point=rng.uniform(0, 1, (B, K, 3)).astype(np.float32), plane_d=rng.uniform(0, 1, (B, K)).astype(np.float32))  # fmt: skip
    ell = EllipsoidLimit.make(2, [0.1, 0.2, 0.0], 0, [0.2, 0.3, 0.4], [-60.0, 45.0, 90.0], [0.8, 0.9, 1.3], weight=4.0)
    parents = np.repeat(np.asarray(c["cons"].pos_parent, np.int32)[None], B, axis=0)
    parents[1, 0] = 2
    variants = {
        "joint-constraint block": (lambda: _problem(c, cons=_with(c["cons"], orc, joint_blocks=[plane])), None),
        "ellipsoid": (lambda: _problem(c, cons=_with(c["cons"], orc, ellipsoid_limits=[ell])), None),
        "per-instance constraint parents": (lambda: _problem(c), lambda pb: pb.set_instance_parents(pos_parent=parents)),
    }
    theta = torch.from_numpy(c["theta"]).to("cuda")
    for key, (make, after) in variants.items():
        pb = make()
        if after is not None:
            after(pb)
        grad = torch.full((B, rig.num_params), -77.0, dtype=torch.float32, device=pb.device)
        err = torch.full((B,), -77.0, dtype=torch.float64, device=pb.device)
        with pytest.raises(capi.MmxError) as ei:
            pb.eval_gradient(theta, grad=grad, err=err)
        torch.cuda.synchronize()
        assert ei.value.code == MMX_ERR_UNSUPPORTED, (key, ei.value)
        assert key in str(ei.value) and "mmx_eval_gradient" in str(ei.value), (key, str(ei.value))
        assert bool((grad == -77.0).all()) and bool((err == -77.0).all()), key
        pb.eval_jacobian(theta)  # the Jacobian path still takes the problem
        torch.cuda.synchronize()


def test_replays_from_a_captured_graph_on_new_parameters(torch_cuda):
    torch = torch_cuda
    c = _case("humanoid72")
    pb = _problem(c)
    B, P, dev = c["B"], c["rig"].num_params, pb.device
    th1 = (c["theta"] + np.float32(0.05) * np.random.default_rng(3).uniform(-1, 1, size=(B, P))).astype(np.float32)
    direct = [_eval(torch, pb, th) for th in (c["theta"], th1)]  # (also the warm-up: the LDS limit is set before the capture)
    theta = torch.from_numpy(c["theta"].copy()).to(dev)
    theta_in = theta.clone()
    grad = torch.zeros((B, P), dtype=torch.float32, device=dev)
    err = torch.zeros((B,), dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            theta.copy_(theta_in)
            pb.eval_gradient(theta, grad=grad, err=err)
    torch.cuda.current_stream().wait_stream(side)
    for th, ref in ((c["theta"], direct[0]), (th1, direct[1]), (c["theta"], direct[0])):
        theta_in.copy_(torch.from_numpy(th.copy()).to(dev))
        grad.zero_()
        err.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(grad.cpu().numpy(), ref[0]) and np.array_equal(err.cpu().numpy(), ref[1])


def test_solver2_matrix_free_agrees_with_its_default_path(torch_cuda, orc):
    """SkeletonSolverFunction.get_gradient / get_error with matrix_free=True against the defaults (the Jacobian contracted on
    the host): the bound of the module docstring, from the oracle's float deviation on the same inputs, with the default path's
    values where g64 / e64 stood.  Element 0's constraints of the 3-joint case at the case's five parameter vectors."""
    from momentum_amd import solver2 as s2

    c = _case("char3")
    ci, rig = c["cons"].instance(0), c["rig"]
    ch = s2.Character(rig)
    pos, ori = s2.PositionErrorFunction(ch), s2.OrientationErrorFunction(ch)
    pos.add_constraints(parent=ci.pos_parent, target=ci.pos_target, offset=ci.pos_offset, weight=ci.pos_weight)
    ori.add_constraints(target=ci.ori_target, parent=ci.ori_parent, offset=ci.ori_offset, weight=ci.ori_weight)
    fn = s2.SkeletonSolverFunction(ch, [pos, ori])
    mp = c["theta"]
    g_def, e_def = fn.get_gradient(mp), fn.get_error(mp)
    g_mf, e_mf = fn.get_gradient(mp, matrix_free=True), fn.get_error(mp, matrix_free=True)
    assert g_mf.shape == g_def.shape == mp.shape and e_mf.shape == e_def.shape == (mp.shape[0],)
    B, P = mp.shape
    g64, g32, e64, e32 = np.zeros((B, P)), np.zeros((B, P), np.float32), np.zeros(B), np.zeros(B)
    for b in range(B):
        J, r, e = orc.eval_jacobian(rig, ci, mp[b].astype(np.float64), None, "f64")
        g64[b], e64[b] = 2.0 * (J.T @ r), e
        Jf, rf, ef = orc.eval_jacobian(rig, ci, mp[b], None, "f32")
        g32[b], e32[b] = np.float32(2.0) * (np.ascontiguousarray(Jf.T) @ rf), ef
    gd = np.asarray(g_def, np.float64)
    _check("solver2 matrix_free vs default", g_mf, e_mf, (gd, e_def, gd + (g32.astype(np.float64) - g64), e_def + (e32 - e64)))
    assert np.isscalar(fn.get_error(mp[0], matrix_free=True)) or isinstance(fn.get_error(mp[0], matrix_free=True), float)
    assert fn.get_gradient(mp[0], matrix_free=True).shape == (P,)
    # outside the scope the library's error comes through: never a fallback to the Jacobian path
    plane = s2.PlaneErrorFunction(ch)
    plane.add_constraints(normal=np.tile([0.0, 1.0, 0.0], (1, 1)), d=np.array([0.5]), parent=[1])
    fn.add_error_function(plane)
    with pytest.raises(capi.MmxError) as ei:
        fn.get_gradient(mp, matrix_free=True)
    assert ei.value.code == MMX_ERR_UNSUPPORTED
    assert fn.get_gradient(mp).shape == mp.shape
