"""The explicit-Jacobian route (MMX_ROUTE_EXPLICIT_JACOBIAN, and mmx_eval_normal_equations on the same kernels) on every
form of its two dispatchers and on both sides of every hand-over between them: launchNormalEquations (normalEquationsKernel
below 32 and above 384 solved parameters, the eight normalEquationsMfmaKernel<TPW, kVec> instantiations with and without
16-byte pieces, the second pass over J from n = 305) and launchCholeskyStep (choleskyStepKernel below and above the default
64 KB of dynamic LDS, choleskyStepTiledKernel<2> with 32 and 16 rows of J per chunk, choleskyStepTiledKernel<kNeCols> with
and without the in-place fetch, the refinement's scalar loads and ragged last chunk), each also with stepUpdateKernel behind
it.  tests/explicit_route_forms.py names the shapes -- one 812-parameter rig, mmx_problem_set_enabled chooses n, 3600, 3597
or 3591 rows choose M modulo 4 / 16 / 32 -- and tests/test_explicit_route_forms_host.py holds, without a GPU, that they reach the
forms and that the oracle's own float solve stays inside the bounds below.

References: the oracle's double J and r (H = J[:, E]^T J[:, E], g = J[:, E]^T r in numpy float64) and its double solve.
Bounds: H and g within 2e-5 of their largest entry and the error within 2e-5 relative (what
test_normal_equations_of_812_parameters holds on this rig), H bit-symmetric, instance 2 (= instance 0) bit-identical to it;
the solve's status and iteration counts equal, the error history within 1e-4 |href| + 1e-7 href[0], theta within
max(1e-5, 3 x sensitivity) relative, disabled parameters untouched bit for bit.

Measured (MI355X; profiles/explicit_route_forms.json has every form): worst H 2e-06, g 1.8e-06, error 1.1e-06 of their
references (the float32 numpy product of the rounded J: H 2.6e-07, g 2.3e-07); theta 1.9e-06 (the float oracle: 7.1e-06),
error history 0.06 of its bound.
"""
import json

import numpy as np
import pytest

from momentum_amd._abi import MMX_STEP_LM_SCHEDULE
from tests import explicit_route_forms as F
from tests.test_gpu_parity import _gpu_problem, _sensitivity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(torch_cuda):
    """One problem handle per constraint set (set_enabled and the route are set per case)."""
    out = {}
    for name in F.CONSTRAINT_SETS:
        cons, _ = F.constraint_set(name)
        rh, pb = _gpu_problem(torch_cuda, F.rig812(), cons, F.B)
        assert pb.M == F.CONSTRAINT_SETS[name]
        out[name] = (rh, pb)
    return out


_ne_cache = {}


def _ne_reference(orc, name):
    """theta in +-0.2 (row 2 = row 0) and the oracle's double J, r, error per instance: once per constraint set."""
    if name not in _ne_cache:
        cons, _ = F.constraint_set(name)
        theta = np.random.default_rng(31 + F.CONSTRAINT_SETS[name]).uniform(-0.2, 0.2, size=(F.B, F.P812)).astype(np.float32)
        theta[2] = theta[0]
        _ne_cache[name] = (theta, [orc.eval_jacobian(F.rig812(), cons.instance(b), theta[b].astype(np.float64), dtype="f64") for b in range(F.B)])
    return _ne_cache[name]


@pytest.mark.parametrize("name,n", F.NE_CASES, ids=[f"{name}-n{n}" for name, n in F.NE_CASES])
def test_normal_equations_form(torch_cuda, orc, handles, name, n):
    torch = torch_cuda
    _, pb = handles[name]
    form = F.ne_form(n, pb.M)
    en = F.enabled_set(n)
    E = np.flatnonzero(en)
    pb.set_enabled(en)
    assert pb.n == n
    theta, ref = _ne_reference(orc, name)
    jtj, jtr, err = pb.normal_equations(torch.from_numpy(theta.copy()).to(pb.device))
    jtj, jtr, err = jtj.cpu().numpy(), jtr.cpu().numpy(), err.cpu().numpy()
    assert jtj.shape == (F.B, n, n) and jtr.shape == (F.B, n)
    worst = dict(H=0.0, g=0.0, err=0.0, H_f32_numpy=0.0, g_f32_numpy=0.0)
    checks = []
    for b in range(F.B):
        J, r, e = ref[b]
        Je = J[:, E]
        H, g = Je.T @ Je, Je.T @ r
        # what single precision itself loses at this n and M: the float32 numpy product of the float-rounded J
        J32, r32 = Je.astype(np.float32), r.astype(np.float32)
        worst["H_f32_numpy"] = max(worst["H_f32_numpy"], np.abs(J32.T @ J32 - H).max() / np.abs(H).max())
        worst["g_f32_numpy"] = max(worst["g_f32_numpy"], np.abs(J32.T @ r32 - g).max() / np.abs(g).max())
        dH, dg, de = np.abs(jtj[b] - H).max() / np.abs(H).max(), np.abs(jtr[b] - g).max() / np.abs(g).max(), abs(err[b] - e) / e
        worst["H"], worst["g"], worst["err"] = max(worst["H"], dH), max(worst["g"], dg), max(worst["err"], de)
        checks.append((np.isfinite(jtj[b]).all() and np.isfinite(jtr[b]).all() and np.isfinite(err[b]), dH, dg, de, np.array_equal(jtj[b], jtj[b].T)))
    print("FORMS " + json.dumps(dict(test="normal_equations", set=name, n=n, form=list(form), **{k: float(v) for k, v in worst.items()})))
    for b, (finite, dH, dg, de, symmetric) in enumerate(checks):
        assert finite, (form, b)
        assert dH <= 2e-5, (form, b, dH)
        assert dg <= 2e-5, (form, b, dg)
        assert de <= 2e-5, (form, b, de)
        assert symmetric, (form, b)  # the mirror store
    # instance stride, no cross-instance state: the same instance twice gives the same bits
    assert np.array_equal(jtj[0], jtj[2]) and np.array_equal(jtr[0], jtr[2]) and err[0] == err[2], form


class _EnabledOracle:
    """The oracle with a shape's enabled set (and one thread per instance) filled in: what _sensitivity calls."""

    def __init__(self, orc, enabled):
        self._orc, self._enabled = orc, enabled

    def solve_batch(self, *args, **kwargs):
        return self._orc.solve_batch(*args, enabled=self._enabled, nthreads=F.B, **kwargs)


def _solve_and_check(torch, orc, pb, name, n, rule):
    form = (F.step_form(n, pb.M), F.step_vec4(pb.M))
    opt = F.solve_options(rule)
    en = F.solve_enabled(name, n)
    off = en == 0
    th0 = F.solve_start(name, n)
    ref = F.oracle_solve(name, n, rule, "f64")
    pb.set_enabled(en)
    assert pb.n == n
    pb.set_route("explicit_jacobian")
    try:
        out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt, want_history=True)
        assert pb.last_route() == "explicit_jacobian"
    finally:
        pb.set_route("auto")
    th = out["theta"].cpu().numpy()
    status, iterations = out["status"].cpu().numpy(), out["iterations"].cpu().numpy()
    h, href = out["error_history"].cpu().numpy(), ref["error_history"]
    rel = F.theta_distance(th, ref["theta"])
    with np.errstate(invalid="ignore", divide="ignore"):
        hist = float(np.nanmax(np.abs(h - href) / (1e-4 * np.abs(href) + 1e-7 * href[:, :1])))
    rel32 = F.theta_distance(F.oracle_solve(name, n, rule, "f32")["theta"], ref["theta"])
    print("FORMS " + json.dumps(dict(test="solve", rule=rule, set=name, n=n, form=[list(form[0]), form[1]], theta=float(rel.max()), history=hist,
                                     theta_f32_oracle=float(rel32.max()), iterations=iterations.tolist())))  # fmt: skip
    assert np.isfinite(th).all() and np.isfinite(h).all()
    assert np.array_equal(status & 3, ref["status"]), (form, status)
    if opt.step_rule != MMX_STEP_LM_SCHEDULE:  # (as in test_wide_solve_variants_agree_with_the_oracle)
        assert np.array_equal(iterations, ref["iterations"]), (form, iterations, ref["iterations"])
    assert np.all(F.history_within_bound(h, href)), (form, hist, h, href)
    tol = np.full(F.B, 1e-5)
    if np.any(rel > tol):  # (the sensitivity costs three more double solves: measured only where 1e-5 alone does not hold)
        cons, _ = F.constraint_set(name)
        tol = np.maximum(tol, 3.0 * _sensitivity(_EnabledOracle(orc, en), F.rig812(), cons, th0, opt, ref))
    assert np.all(rel <= tol), (form, rel, tol)
    assert np.array_equal(th[:, off], th0[:, off]), form  # disabled parameters: bit-identical to the start


@pytest.mark.parametrize("name,n", F.SOLVE_CASES, ids=[f"{name}-n{n}" for name, n in F.SOLVE_CASES])
def test_pinned_solve_form(torch_cuda, orc, handles, name, n):
    """Three iterations on the pinned route; element 1 starts at its solution, is done after its first convergence test and
    sits out the last iteration: the `done` gate of every kernel runs."""
    _solve_and_check(torch_cuda, orc, handles[name][1], name, n, "plain")


@pytest.mark.parametrize("n,rule", F.DEFERRED_CASES, ids=[f"n{n}-{rule}" for n, rule in F.DEFERRED_CASES])
def test_deferred_step_form(torch_cuda, orc, handles, n, rule):
    """stepUpdateKernel behind each step form (the directional line search, the LM schedule; four iterations) on the 3597-row
    set: scalar loads and a ragged last chunk in the tiled refinement."""
    _solve_and_check(torch_cuda, orc, handles["M3597"][1], "M3597", n, rule)
