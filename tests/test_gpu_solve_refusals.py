"""The refusals of the solve dispatch (mmx_solve*, mmx_solve_frames; planned in momentum_amd/csrc/mmx_solve_plan.cpp), one by
one: the status code and the FULL message, theta and every passed output array bit-unchanged (the outputs carry a sentinel),
and mmx_problem_last_route as the accepted solve before the refused call left it.  Every call returns before a launch.

Shapes: the 3-joint reference rig and the 24-joint chain of tests/test_gpu_wave_route.py at B = 2 (frames: B = 4, two frames) --
the smallest at which each of these refusals is reachable.  Refusals other tests assert with the same strength are not repeated
(more than 2048 parameters: test_gpu_many_parameters.py; the wave route's scope conditions: test_gpu_wave_route_edges.py)."""
import numpy as np
import pytest

from momentum_amd import capi, make_test_character
from momentum_amd._abi import (MMX_PRECISION_AUTO, MMX_PRECISION_F32, MMX_PRECISION_F64, MMX_PRECISION_MIXED, MMX_STEP_GN_FIXED_LAMBDA,
                               MMX_STEP_LM_SCHEDULE, MMX_STEP_TRUST_REGION, GnOptions, ParameterLimit)  # fmt: skip
from tests.helpers import make_problem
from tests.test_gpu_wave_route import _all_joints, _problem

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4  # MMX_ERR_INVALID_ARGUMENT, MMX_ERR_UNSUPPORTED
FIXED = dict(min_iterations=3, max_iterations=3, threshold=1.0, regularization=0.05)
PRECISIONS = {"f32": MMX_PRECISION_F32, "f64": MMX_PRECISION_F64, "auto": MMX_PRECISION_AUTO, "mixed": MMX_PRECISION_MIXED}

ITERATIONS = "iteration counts must be >= 0"
STEP_RULE = "unknown step_rule"
LINE_SEARCH = "unknown do_line_search rule"
PRECISION = "unknown precision (MMX_PRECISION_*)"
STEP_HISTORY = "mmx_solve_with_step_history: step_history is the LM schedule's (MMX_STEP_LM_SCHEDULE)"
PARAMETER_HISTORY = ("parameter_history is single precision's (MMX_PRECISION_F32) and the mixed-precision instantiation's: the double "
                     "instantiation does not record it")  # fmt: skip
WAVE_PRECISION = "MMX_ROUTE_WAVE: only MMX_PRECISION_F32 (not F64 / AUTO / MIXED)"
WAVE_STEP_RULE = "MMX_ROUTE_WAVE: only MMX_STEP_GN_FIXED_LAMBDA (not the LM schedule, not the trust region)"
TRUST_REGION = ("MMX_STEP_TRUST_REGION: available in the one-launch solve and on the wide route (tree kernels); this problem takes neither "
                "(MMX_ROUTE_EXPLICIT_JACOBIAN, or outside the tree kernels' scope)")  # fmt: skip
WIDE_SCOPE = "MMX_ROUTE_WIDE: the problem is outside the tree kernels' scope"
FRAMES_COUNT = "mmx_solve_frames: num_frames must be >= 1 and divide the problem's batch (num_frames x sequences instances, frame-major)"
FRAMES_PRECISION = "mmx_solve_frames runs on MMX_ROUTE_WAVE: only MMX_PRECISION_F32 (not F64 / AUTO / MIXED)"
FRAMES_ROUTE = ("mmx_solve_frames runs on the one-wavefront route only: the handle's route is pinned to another (MMX_ROUTE_AUTO or "
                "MMX_ROUTE_WAVE)")  # fmt: skip


def _make(torch, joints, B, route, pos=True, **kw):
    rig = make_test_character(joints)
    jj = _all_joints(rig) if pos else []
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
    return _problem(torch, rig, cons, B, route=route, **kw), th0


def _accepted(torch, pb, th0, frames=0):
    t = torch.from_numpy(th0.copy()).to(pb.device)
    out = pb.solve_frames(t, GnOptions.make(**FIXED), frames) if frames else pb.solve(t, GnOptions.make(**FIXED))
    torch.cuda.synchronize()
    assert np.all(out["status"].cpu().numpy() & 3 == 0)
    return pb.last_route()


def _refused(torch, pb, th0, opt, code, message, histories=("error_history",), frames=None):
    """One refused call: code and message, nothing written, the recorded route kept."""
    B, P, K = pb.B, pb.P, max(1, opt.max_iterations)
    route = pb.last_route()
    theta = torch.from_numpy(th0.copy()).to(pb.device)
    shapes = dict(error=((B,), torch.float64), iterations=((B,), torch.int32), status=((B,), torch.int32), error_history=((B, K), torch.float64),
                  parameter_history=((B, K, P), torch.float32), step_history=((B, K, 2), torch.float64))  # fmt: skip
    outputs = {k: torch.full(shp, -7, dtype=dt, device=pb.device) for k, (shp, dt) in shapes.items() if k in ("error", "iterations", "status") + tuple(histories)}
    before = {k: v.cpu().numpy().copy() for k, v in outputs.items()}
    with pytest.raises(capi.MmxError) as ei:
        if frames is None:
            pb.solve(theta, opt, outputs=outputs)
        else:
            pb.solve_frames(theta, opt, frames, outputs=outputs)
    got = (ei.value.code, str(ei.value))
    del ei  # (the traceback holds this frame, and with it the handle: no reference cycle is left for the collector to take apart)
    assert got == (code, f"mmx error {code}: {message}")
    torch.cuda.synchronize()
    assert np.array_equal(theta.cpu().numpy(), th0)
    for k, v in before.items():
        assert np.array_equal(outputs[k].cpu().numpy(), v), k
    assert pb.last_route() == route


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_option_checks_under_every_precision(torch_cuda, precision):
    pb, th0 = _make(torch_cuda, 24, 2, "auto")
    _accepted(torch_cuda, pb, th0)
    p = PRECISIONS[precision]
    for kw, message in ((dict(max_iterations=-1), ITERATIONS), (dict(min_iterations=-1), ITERATIONS), (dict(step_rule=7), STEP_RULE),
                        (dict(do_line_search=5), LINE_SEARCH)):  # fmt: skip
        _refused(torch_cuda, pb, th0, GnOptions.make(**{**FIXED, **kw}, precision=p), INVALID, message)


def test_unknown_precision_and_the_histories(torch_cuda):
    pb, th0 = _make(torch_cuda, 24, 2, "auto")
    _accepted(torch_cuda, pb, th0)
    _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=9), INVALID, PRECISION)
    for rule in (MMX_STEP_GN_FIXED_LAMBDA, MMX_STEP_TRUST_REGION):
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, step_rule=rule), INVALID, STEP_HISTORY, histories=("error_history", "step_history"))
    # (the step-history check comes first, whatever else is wrong with the call)
    _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=9), INVALID, STEP_HISTORY, histories=("step_history",))
    for p in (MMX_PRECISION_F64, MMX_PRECISION_AUTO):
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=p), UNSUPPORTED, PARAMETER_HISTORY, histories=("error_history", "parameter_history"))


def test_pinned_wave_route(torch_cuda):
    pb, th0 = _make(torch_cuda, 24, 2, "wave")
    assert _accepted(torch_cuda, pb, th0) == "wave"
    for p in (MMX_PRECISION_F64, MMX_PRECISION_AUTO, MMX_PRECISION_MIXED):
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=p), UNSUPPORTED, WAVE_PRECISION)
        # (... before the step rule is looked at)
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=p, step_rule=MMX_STEP_LM_SCHEDULE), UNSUPPORTED, WAVE_PRECISION)
    for rule in (MMX_STEP_LM_SCHEDULE, MMX_STEP_TRUST_REGION):
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, step_rule=rule), UNSUPPORTED, WAVE_STEP_RULE, histories=("error_history", "parameter_history"))
    _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, step_rule=MMX_STEP_LM_SCHEDULE), UNSUPPORTED, WAVE_STEP_RULE, histories=("step_history",))


def test_trust_region_with_the_explicit_jacobian_route_pinned(torch_cuda):
    pb, th0 = _make(torch_cuda, 3, 2, "explicit_jacobian")
    assert _accepted(torch_cuda, pb, th0) == "explicit_jacobian"
    _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, step_rule=MMX_STEP_TRUST_REGION), UNSUPPORTED, TRUST_REGION, histories=("error_history", "parameter_history"))


def test_wide_route_pinned_outside_the_tree_kernels_scope(torch_cuda):
    """No position / orientation constraint (a parameter limit only): the tree kernels have nothing to sum."""
    pb, th0 = _make(torch_cuda, 3, 2, "auto", pos=False, limits=[ParameterLimit.minmax(1, -0.05, 0.05, 2.0)])
    _accepted(torch_cuda, pb, th0)
    pb.set_route("wide")
    for rule in (MMX_STEP_GN_FIXED_LAMBDA, MMX_STEP_LM_SCHEDULE, MMX_STEP_TRUST_REGION):
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, step_rule=rule), UNSUPPORTED, WIDE_SCOPE, histories=("error_history", "parameter_history"))


def test_solve_frames_entry_conditions(torch_cuda):
    pb, th0 = _make(torch_cuda, 24, 4, "auto")
    assert _accepted(torch_cuda, pb, th0, frames=2) == "wave"
    opt = GnOptions.make(**FIXED)
    hist = ("error_history", "parameter_history")
    for frames in (3, 0, -2, 8):
        _refused(torch_cuda, pb, th0, opt, INVALID, FRAMES_COUNT, histories=hist, frames=frames)
    _refused(torch_cuda, pb, th0, GnOptions.make(**{**FIXED, "max_iterations": -1}), INVALID, ITERATIONS, histories=hist, frames=2)
    _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, do_line_search=5), INVALID, LINE_SEARCH, histories=hist, frames=2)
    for p in (MMX_PRECISION_F64, MMX_PRECISION_AUTO, MMX_PRECISION_MIXED, 9):
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=p), UNSUPPORTED, FRAMES_PRECISION, histories=hist, frames=2)
    # the step rule is the wave route's to refuse, an unknown one included
    for rule in (MMX_STEP_LM_SCHEDULE, MMX_STEP_TRUST_REGION, 7):
        _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, step_rule=rule), UNSUPPORTED, WAVE_STEP_RULE, histories=hist, frames=2)
    for route in ("fused", "wide", "explicit_jacobian"):
        pb.set_route(route)
        _refused(torch_cuda, pb, th0, opt, UNSUPPORTED, FRAMES_ROUTE, histories=hist, frames=2)
    # (num_frames is looked at before the precision, the precision before the route)
    _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=MMX_PRECISION_F64), INVALID, FRAMES_COUNT, histories=hist, frames=3)
    _refused(torch_cuda, pb, th0, GnOptions.make(**FIXED, precision=MMX_PRECISION_F64), UNSUPPORTED, FRAMES_PRECISION, histories=hist, frames=2)
