"""MMX_ROUTE_WAVE (momentum_amd/csrc/mmx_wave.hip) where its layout decisions change, pinned, against the oracle's DOUBLE
instantiation: joints in lanes up to the last one (J = 33, 63, 64; a 64-joint chain runs the sixth pointer-jumping round), units in
lanes with stride 64 (U = 1, 64, 65, 128, 129, 191, 192: every pass empty / full / one over), both system sizes at their ends
(n = 1, 15, 16 in the 16-column instantiation, 17, 31, 32 in the 32-column one).  The inputs are tests/test_wave_route_edge_inputs.py's
72-case grid (B = 5: two workgroups, three idle waves).

Bounds.  All of them come from the oracle's own FLOAT instantiation against its double one on these inputs, measured on the CPU --
none from the kernel:
  (a) one step (min = max = 1, lambda 0.5, no line search): |theta_1 - ref_1| / max(|ref_1 - theta_0|, 1e-3) <= max(3e-5, 3 x the float
      oracle's same distance) per instance; error_history[:, 0] (FK + units at theta_0) within 1e-6 relative of the double oracle's --
      3 x the float oracle's distance on a case where the float oracle itself is outside 1e-6.  A whole solve repairs a wrong entry
      of H in its later iterations; the first step on its own does not.
  (b) five iterations with the case's line-search rule: |theta - ref| / max(|ref|, 1e-3) <= max(2e-5, 3 x float oracle), iterations and
      status & 3 equal, error history within 1e-4 max(1, |h|), disabled columns bit-equal to theta_0.
A case is WIDENED when it needs more than the base bound (3e-5 / 2e-5), or when its error bound at theta_0 is the float oracle's; at
most 9 of the 72 cases may be, in each of (a) and (b) -- the float oracle alone needs fewer (asserted on the CPU by
tests/test_wave_route_edge_inputs.py).  No case is skipped or exempted.  (The generator draws a case again when the double replay
of its line search has an accept / reject decision closer than one float ulp of the error -- see the inputs file: decided from the
double reference alone.)

Beyond the grid: each limit of the route refused on its own (65 joints, 33 solved parameters, 193 units: the others at their
maximum), the parameter history, per-instance pre-rotations, and MMX_SOLVE_DAMPING_FLOORED (status bit 4) on both sides of the
floor.  The fourth refusal, a parameter vector that does not fit a wave's share of LDS, cannot be built: a rig has at most 2048
parameters (kMaxModelParams), and 2 x 2048 + 17 x 64 + 8 x 192 + 32 x 36 + 32 = 7904 floats per wave stay under the 10240 a quarter of
160 KB holds -- inside the other limits the condition is unreachable."""
import copy
import ctypes as C

import numpy as np
import pytest

from momentum_amd import capi, make_test_character
from momentum_amd._abi import GnOptions
from tests.helpers import make_problem
from tests.test_gpu_fuzz import random_rig
from tests.test_gpu_wave_route import _expect_unsupported, _problem, _rel, _solve
from tests.test_wave_route_edge_inputs import (BATCH, ERR0_BOUND, MAX_WIDENED, NUM_CASES, SOLVE_BOUND, STEP_BOUND, edge_case, err0_distance,
                                               grid_index, per_instance_case, pick_enabled, reference, step_distance)  # fmt: skip

pytestmark = pytest.mark.gpu
KEYS = ("theta", "error", "iterations", "status", "error_history")


def _solved_count(pb):
    """The solved count after the library's structural-zero elimination (the size query of mmx_debug_fused_normal_equations)."""
    n = C.c_int32(-1)
    rc = capi.lib().mmx_debug_fused_normal_equations(pb._h, None, None, None, None, C.byref(n), None)
    assert rc == 0
    return n.value


def _grid_problem(torch, c):
    pb = _problem(torch, c.rig, c.cons, BATCH)
    pb.set_enabled(c.enabled)
    assert _solved_count(pb) == c.n
    return pb


def _tag(c):
    return "case %2d J %2d %-5s n %2d U %3d ls %d" % (c.k, c.J, c.shape, c.n, c.U, c.line_search)


ROWS_A, ROWS_B, WIDENED_A, WIDENED_B = {}, {}, [], []


@pytest.mark.parametrize("k", range(NUM_CASES))
def test_grid_one_step(torch_cuda, k):
    c, r = edge_case(k), reference(k)
    pb = _grid_problem(torch_cuda, c)
    out = _solve(torch_cuda, pb, c.th0, c.one_step)
    assert pb.last_route() == "wave"
    ref = r.one_f64
    d = step_distance(out["theta"], ref["theta"], c.th0)
    e0 = err0_distance(out["error_history"], ref["error_history"])
    tol_e = np.full(BATCH, ERR0_BOUND)
    widened = False
    if np.any(r.err0_32 > ERR0_BOUND):  # the float oracle itself is outside 1e-6 here
        tol_e = np.maximum(tol_e, 3.0 * r.err0_32)
        widened = True
    tol = np.full(BATCH, STEP_BOUND)
    if np.any(d > tol):
        tol = np.maximum(tol, 3.0 * r.step32)
        widened = True
    if widened:
        WIDENED_A.append(k)
    ROWS_A[k] = "%s | step: gpu %.2e float oracle %.2e | error at theta0: gpu %.2e float oracle %.2e%s" % (
        _tag(c), d.max(), r.step32.max(), e0.max(), r.err0_32.max(), " WIDENED" if widened else "")  # fmt: skip
    print(ROWS_A[k], "| widened so far", WIDENED_A)
    assert len(WIDENED_A) <= MAX_WIDENED, WIDENED_A
    assert np.all(d <= tol), (k, d, tol)
    assert np.all(e0 <= tol_e), (k, e0, tol_e)
    assert np.all(out["iterations"] == 1) and np.array_equal(out["status"] & 3, ref["status"])
    assert np.all(out["theta"][:, c.enabled == 0] == c.th0[:, c.enabled == 0])


@pytest.mark.parametrize("k", range(NUM_CASES))
def test_grid_five_iterations(torch_cuda, k):
    c, r = edge_case(k), reference(k)
    pb = _grid_problem(torch_cuda, c)
    out = _solve(torch_cuda, pb, c.th0, c.five)
    assert pb.last_route() == "wave"
    ref = r.five_f64
    rel = _rel(out["theta"], ref["theta"])
    tol = np.full(BATCH, SOLVE_BOUND)
    widened = bool(np.any(rel > tol))
    if widened:
        tol = np.maximum(tol, 3.0 * r.solve32)
        WIDENED_B.append(k)
    ROWS_B[k] = "%s | five iterations: gpu %.2e float oracle %.2e%s" % (_tag(c), rel.max(), r.solve32.max(), " WIDENED" if widened else "")
    print(ROWS_B[k], "| widened so far", WIDENED_B)
    assert len(WIDENED_B) <= MAX_WIDENED, WIDENED_B
    assert np.all(rel <= tol), (k, rel, tol)
    assert np.array_equal(out["iterations"], ref["iterations"])
    assert np.array_equal(out["status"] & 3, ref["status"])
    h, href = out["error_history"], ref["error_history"]
    assert np.abs(h - href).max() <= 1e-4 * max(1.0, np.abs(href).max())
    assert np.all(out["theta"][:, c.enabled == 0] == c.th0[:, c.enabled == 0])


def test_grid_report():
    """The per-case figures of the two tests above in one place (run after them), and the caps once more."""
    for name, rows, wide in (("(a) one step", ROWS_A, WIDENED_A), ("(b) five iterations", ROWS_B, WIDENED_B)):
        print("\n%s: %d cases, widened %s" % (name, len(rows), wide))
        for k in sorted(rows):
            print(rows[k])
        assert len(wide) <= MAX_WIDENED, (name, wide)


def _limit_problem(J, n, Kp, Ko, seed):
    rng = np.random.default_rng(seed)
    rig = random_rig(rng, J, "bushy")
    pp = rng.integers(0, J, size=Kp).astype(np.int32)
    op = rng.integers(0, J, size=Ko).astype(np.int32)
    pp[0] = J - 1
    cons, th0, _ = make_problem(rig, pp, op, BATCH, seed=seed, perturb=0.25, random_offsets=True, weights="random")
    return rig, cons, th0, pick_enabled(rig, cons, th0, n)


def _refused_with(torch, pb, th0, opt, needle):
    _expect_unsupported(torch, pb, th0, opt)  # MMX_ERR_UNSUPPORTED, theta untouched
    with pytest.raises(capi.MmxError) as ei:
        pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt)
    assert needle in str(ei.value), str(ei.value)
    for other in ("MMX_WAVE_MAX_JOINTS", "MMX_WAVE_MAX_SOLVED", "MMX_WAVE_MAX_UNITS", "does not fit"):
        assert other == needle or other not in str(ei.value), str(ei.value)


@pytest.mark.parametrize("limit", ["joints", "solved", "units"])
def test_refusals_one_limit_at_a_time(torch_cuda, limit):
    """Only the named limit is crossed, by one; the other two sit AT their maximum (64 joints, 32 solved, 192 units)."""
    torch = torch_cuda
    opt = GnOptions.make(min_iterations=2, max_iterations=2, regularization=0.5)
    J, n, Kp, Ko, needle = {"joints": (65, 32, 63, 43, "MMX_WAVE_MAX_JOINTS"), "solved": (64, 33, 63, 43, "MMX_WAVE_MAX_SOLVED"),
                            "units": (64, 32, 64, 43, "MMX_WAVE_MAX_UNITS")}[limit]  # fmt: skip
    rig, cons, th0, en = _limit_problem(J, n, Kp, Ko, seed=9500 + len(limit))
    pb = _problem(torch, rig, cons, BATCH)
    pb.set_enabled(en)
    assert _solved_count(pb) == n and cons.Kp + 3 * cons.Ko == (193 if limit == "units" else 192) and rig.num_joints == J
    _refused_with(torch, pb, th0, opt, needle)
    if limit == "solved":  # the condition lifted on the same handle: one parameter fewer
        en[np.flatnonzero(en)[-1]] = 0
        pb.set_enabled(en)
        assert _solved_count(pb) == 32
        out = _solve(torch, pb, th0, opt)
        assert pb.last_route() == "wave" and np.all(out["status"] & 3 == 0) and np.all(out["iterations"] == 2)
        assert np.all(out["theta"][:, en == 0] == th0[:, en == 0]) and np.any(out["theta"] != th0)


def _history_inputs(name):
    if name == "chain24":
        rig = make_test_character(24)
        jj = np.arange(rig.num_joints, dtype=np.int32)
        cons, th0, _ = make_problem(rig, jj, jj, 8, seed=12345, perturb=0.3)
        return rig, cons, th0, None, 0.05
    c = edge_case(grid_index(64, "bushy", (32, 63, 43)))
    return c.rig, c.cons, c.th0, c.enabled, 0.5


@pytest.mark.parametrize("line_search", [0, 2])
@pytest.mark.parametrize("name", ["chain24", "grid_n32"])
def test_parameter_history_matches_the_iterates(torch_cuda, orc, name, line_search):
    """SolverT::setStoreHistory on the route (the kernel writes row `it` itself): the last row written is theta, the rows past
    iterations[b] stay zero, row i is bit for bit the theta of a solve truncated at i + 1 iterations -- with the directional line
    search too, where the last trial's state is handed to the next iteration."""
    torch = torch_cuda
    rig, cons, th0, en, lam = _history_inputs(name)
    B = th0.shape[0]
    pb = _problem(torch, rig, cons, B)
    if en is not None:
        pb.set_enabled(en)
    opt = GnOptions.make(min_iterations=2, max_iterations=6, threshold=1e9, regularization=lam, do_line_search=line_search)  # stops after min + 1
    out = _solve(torch, pb, th0, opt, want_parameter_history=True)
    assert pb.last_route() == "wave"
    hist, iters, th = out["parameter_history"], out["iterations"], out["theta"]
    assert hist.shape == (B, 6, rig.num_params) and iters.min() >= 3 and iters.min() < 6  # some element stops early
    assert np.any(th != th0)
    for b in range(B):
        assert np.array_equal(hist[b, iters[b] - 1], th[b])
        assert np.all(hist[b, iters[b]:] == 0)
        assert np.all(out["error_history"][b, iters[b]:] == 0)
    plain = _solve(torch, pb, th0, opt)  # the history is an output, not an input
    for key in KEYS:
        assert np.array_equal(plain[key], out[key]), key
    for i in range(int(iters.min())):
        o2 = GnOptions.make(min_iterations=i + 1, max_iterations=i + 1, threshold=1e9, regularization=lam, do_line_search=line_search)
        ti = _solve(torch, pb, th0, o2)
        assert pb.last_route() == "wave"
        assert np.array_equal(hist[:, i], ti["theta"]), i
        assert i == 0 or np.any(hist[:, i] != hist[:, i - 1])
    ref = orc.solve_batch(rig, cons, th0, opt, enabled=en, dtype="f64")
    assert np.array_equal(iters, ref["iterations"])
    if en is not None:
        assert np.all(hist[:, : iters.min()][:, :, en == 0] == th0[:, None, en == 0])


@pytest.mark.parametrize("mode", ["pre_rotations", "offsets_and_pre_rotations"])
@pytest.mark.parametrize("name", ["chain24", "bushy40"])
def test_per_instance_pre_rotations(torch_cuda, orc, name, mode):
    """set_instance_rig(None, pre) and (off, pre): every element against the oracle on a copy of the rig with that element's
    arrays, at test_per_instance_rigs' bounds."""
    p = per_instance_case(name)
    B = p.th0.shape[0]
    off = p.off if mode == "offsets_and_pre_rotations" else None
    pb = _problem(torch_cuda, p.rig, p.cons, B)
    if p.enabled is not None:
        pb.set_enabled(p.enabled)
    pb.set_instance_rig(off, p.pre)
    out = _solve(torch_cuda, pb, p.th0, p.opt)
    assert pb.last_route() == "wave"
    ps = _problem(torch_cuda, p.rig, p.cons, B)
    if p.enabled is not None:
        ps.set_enabled(p.enabled)
    shared = _solve(torch_cuda, ps, p.th0, p.opt)
    worst = 0.0
    for b in range(B):
        rb = copy.deepcopy(p.rig)
        rb.pre_rotation[:] = p.pre[b]
        if off is not None:
            rb.translation_offset[:] = off[b]
        ref = orc.solve(rb, p.cons.instance(b), p.th0[b], p.opt, enabled=p.enabled, dtype="f64")
        rel = np.linalg.norm(out["theta"][b] - ref["theta"]) / max(np.linalg.norm(ref["theta"]), 1e-3)
        worst = max(worst, rel)
        assert rel <= 1e-5, (b, rel)
        assert int(out["iterations"][b]) == ref["iterations"] and int(out["status"][b]) & 3 == ref["status"]
        href = np.asarray(ref["error_history"])
        assert np.abs(out["error_history"][b][: len(href)] - href).max() <= 1e-4 * max(1.0, np.abs(href).max())
        # the element's arrays are what was used, not the shared rig's
        assert np.linalg.norm(shared["theta"][b] - ref["theta"]) > 1e-3 * np.linalg.norm(ref["theta"])
    print("%s %s: worst rel %.3e" % (name, mode, worst))
    pb.set_instance_rig(None, None)  # back to the shared rig on the same handle
    again = _solve(torch_cuda, pb, p.th0, p.opt)
    for key in KEYS:
        assert np.array_equal(again[key], shared[key]), key


@pytest.mark.parametrize("nkk,J,shape", [((1, 1, 0), 64, "chain"), ((16, 128, 0), 63, "star"), ((32, 63, 43), 64, "bushy")])
def test_damping_floor_bit(torch_cuda, orc, nkk, J, shape):
    """MMX_SOLVE_DAMPING_FLOORED: what is factored is J^T J + max(lambda, kFactorDamping trace(J^T J) / n).  With
    f = 1e-5 trace / n from the double Jacobian at theta_0, lambda = f / 8 sets the bit in every element and lambda = 8 f in none
    (the factor 8 keeps the float rounding of the kernel's own trace away from the decision); no error bit either way."""
    c = edge_case(grid_index(J, shape, nkk))
    cols = np.flatnonzero(c.enabled)
    f = np.zeros(BATCH)
    for b in range(BATCH):
        Jm, _, _ = orc.eval_jacobian(c.rig, c.cons.instance(b), c.th0[b].astype(np.float64), dtype="f64")
        f[b] = 1e-5 * np.sum(Jm[:, cols] ** 2) / len(cols)
    assert len(cols) == c.n and np.all(f > 0)
    pb = _grid_problem(torch_cuda, c)
    for lam, bit in ((f.min() / 8.0, 4), (8.0 * f.max(), 0)):
        out = _solve(torch_cuda, pb, c.th0, GnOptions.make(min_iterations=1, max_iterations=1, regularization=lam))
        assert pb.last_route() == "wave"
        print("n %d lambda %.3e floor %.3e .. %.3e status %s" % (c.n, lam, f.min(), f.max(), out["status"]))
        assert np.all(out["status"] & 4 == bit), (lam, out["status"])
        assert np.all(out["status"] & 3 == 0), out["status"]
        assert np.all(out["iterations"] == 1) and np.any(out["theta"] != c.th0)
