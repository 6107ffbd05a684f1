"""Inputs of tests/test_gpu_wave_route_edges.py (the boundary grid of MMX_ROUTE_WAVE) and the CPU check that they are what the
grid says: edge_case(k), k = 0 .. 71, is the product of J in {33, 63, 64} joints (lanes = joints: the upper quarter of the wave,
the last lane), three tree shapes (a 64-joint chain has depth 63: the sixth pointer-jumping round) and eight (n, Kp, Ko)
combinations that put the solved count on both sides of the 16 / 32-column instantiations and the unit count U = Kp + 3 Ko on
both sides of every 64-unit pass (1, 64, 65, 128, 129, 191, 192).

The bounds the GPU test holds the kernel to come from the oracle's own FLOAT instantiation against its double one on these very
inputs, measured on the CPU (never from the kernel): a step after one iteration within 3e-5 of the step's length, theta after five
iterations within 2e-5, the error at theta0 within 1e-6 relative; a case where the float oracle itself is outside one of them is
held to 3 x the float oracle's distance instead ("widened"), and at most 9 of the 72 cases may be (the float oracle needs fewer:
asserted below).

Every third case runs a backtracking line search.  A line search decides by comparing two errors, and a decision whose margin is
under one float ulp of the error is not determined in single precision: theta then differs by a whole backtracking factor of the
step whichever arithmetic is right.  The original draw of case 20 (seed k) had such decisions -- rule 1 rejected scale 2^-8 of
iteration 4 short by about 1e-8 of the error; the kernel accepted it and sat 8.2e-5 from the double oracle, exactly where a replay of
the double solve with that one decision flipped sits -- so edge_case() replays the line search in double and draws the problem
(offsets, weights, targets: not the rig, not the grid) again while any decision that matters is closer than DECIDABLE; two of the
72 cases take a second draw.  A change to random_rig / make_problem that empties the grid (wrong n, wrong U, the last lane unconstrained, a
reference that no longer converges) fails here, without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np

from momentum_amd import make_test_character
from momentum_amd._abi import GnOptions
from oracle import oracle as orc
from tests.helpers import make_problem, quat_mul
from tests.test_gpu_fuzz import random_rig

GRID_J = (33, 63, 64)
GRID_SHAPE = ("chain", "star", "bushy")
GRID_NKK = ((1, 1, 0), (15, 1, 21), (16, 64, 0), (17, 65, 0), (16, 128, 0), (17, 129, 0), (31, 62, 43), (32, 63, 43))  # (n, Kp, Ko)
NUM_CASES = len(GRID_J) * len(GRID_SHAPE) * len(GRID_NKK)
BATCH = 5  # two workgroups of four waves, three of them idle
LAMBDA = 0.5
STEP_BOUND, SOLVE_BOUND, ERR0_BOUND, MAX_WIDENED = 3e-5, 2e-5, 1e-6, 9


def grid_index(J, shape, nkk):
    return (GRID_J.index(J) * len(GRID_SHAPE) + GRID_SHAPE.index(shape)) * len(GRID_NKK) + GRID_NKK.index(tuple(nkk))


def live_columns(rig, cons, theta):
    """Parameters whose column of the double Jacobian at theta has a non-zero entry (instance 0 of the batch)."""
    Jm, _, _ = orc.eval_jacobian(rig, cons.instance(0), np.asarray(theta, np.float64), dtype="f64")
    return np.flatnonzero(np.abs(Jm).max(axis=0) > 0)


def pick_enabled(rig, cons, th0, n):
    """Exactly n parameters, evenly spaced among the live columns: the library's structural-zero elimination keeps all of them."""
    live = live_columns(rig, cons, th0[0].astype(np.float64) + 0.1)
    assert len(live) >= n, (len(live), n)
    en = np.zeros(rig.num_params, np.uint8)
    en[live[np.round(np.linspace(0, len(live) - 1, n)).astype(int)]] = 1
    assert int(en.sum()) == n
    return en


def line_search_trace(rig, cons, th0, enabled, rule, iterations=5, lam=LAMBDA):
    """The backtracking line search of the solve, replayed in double on numpy normal-equation steps (the double oracle to 1e-12:
    asserted below).  Returns (theta [B, P], the smallest |decrease - required decrease| / error over every accept / reject decision
    taken): a decision whose margin is under the resolution of a single-precision error sum is not determined in float."""
    cols = np.flatnonzero(enabled)
    out, worst = np.zeros(th0.shape, np.float64), np.inf
    for b in range(th0.shape[0]):
        ci = cons.instance(b)
        th = th0[b].astype(np.float64)
        for _ in range(iterations):
            Jm, res, err = orc.eval_jacobian(rig, ci, th, dtype="f64")
            Jc = Jm[:, cols]
            g = Jc.T @ res
            d = np.linalg.solve(Jc.T @ Jc + lam * np.eye(len(cols)), g)
            scale = 1.0
            for trial in range(10):
                tr = th.copy()
                tr[cols] -= scale * d
                e = orc.eval_jacobian(rig, ci, tr, dtype="f64")[2]
                need = scale * 1e-3 * err if rule == 1 else 1e-4 * scale * (g @ d)  # gauss_newton_solver.cpp / gauss_newton_solver_qr.cpp
                if trial < 9:  # (the tenth trial is taken whatever its decision)
                    worst = min(worst, abs(err - e - need) / err)
                if err - e >= need:
                    break
                scale *= 0.5
            th = tr
        out[b] = th
    return out, worst


# No single-precision evaluation resolves the error better than one ulp of its value (its terms are floats).  An accept / reject
# decision of the line search whose margin, relative to the error, is under that falls either way in float, and theta then differs
# by a whole backtracking factor of the step: not an error of the arithmetic under test.  The generator draws such a problem again.
# (Rule 1 asks for a decrease of 1e-3 x error x scale, which a converged iterate misses at all ten scales: at the last one that
# decides anything, 2^-8, the margin is 4e-6 |1 - decrease / required| of the error -- typically 2e-7 .. 1.6e-6.)
DECIDABLE = float(np.finfo(np.float32).eps)
MAX_REDRAWS = 8


@functools.lru_cache(maxsize=None)
def edge_case(k):
    J = GRID_J[k // (len(GRID_SHAPE) * len(GRID_NKK))]
    shape = GRID_SHAPE[(k // len(GRID_NKK)) % len(GRID_SHAPE)]
    n, Kp, Ko = GRID_NKK[k % len(GRID_NKK)]
    rng = np.random.default_rng(9000 + k)
    rig = random_rig(rng, J, shape)
    pp = rng.integers(0, J, size=Kp).astype(np.int32)
    op = rng.integers(0, J, size=Ko).astype(np.int32)
    pp[0] = J - 1  # the last lane's joint always carries a constraint
    line_search = (1 + (k // 3) % 2) if k % 3 == 2 else 0  # every third case, rules 1 and 2 in turn
    for redraw in range(MAX_REDRAWS + 1):  # (the rig and the constraint parents stay: only offsets, weights and targets are drawn again)
        cons, th0, _ = make_problem(rig, pp, op, BATCH, seed=k + 1000 * redraw, perturb=0.25, random_offsets=True, weights="random")
        en = pick_enabled(rig, cons, th0, n)
        margin = line_search_trace(rig, cons, th0, en, line_search)[1] if line_search else np.inf
        if margin >= DECIDABLE:
            break
    else:
        raise AssertionError("case %d: no draw with every line-search decision decidable in float" % k)
    return SimpleNamespace(k=k, J=J, shape=shape, n=n, Kp=Kp, Ko=Ko, U=Kp + 3 * Ko, rig=rig, cons=cons, th0=th0, enabled=en,
                           line_search=line_search, redraw=redraw, margin=margin,
                           one_step=GnOptions.make(min_iterations=1, max_iterations=1, regularization=LAMBDA),
                           five=GnOptions.make(min_iterations=5, max_iterations=5, regularization=LAMBDA, do_line_search=line_search))  # fmt: skip


def step_distance(th, ref, th0):
    """|theta_1 - ref_1| / max(|ref_1 - theta_0|, 1e-3) per instance: the error of the STEP, relative to its length."""
    return np.linalg.norm(th - ref, axis=1) / np.maximum(np.linalg.norm(ref - th0, axis=1), 1e-3)


def solve_distance(th, ref):
    return np.linalg.norm(th - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-3)


def err0_distance(h, href):
    return np.abs(h[:, 0] - href[:, 0]) / np.maximum(np.abs(href[:, 0]), 1e-30)


@functools.lru_cache(maxsize=None)
def reference(k):
    """The two oracles on case k: (a) one step, (b) five iterations with the case's line-search rule, and the float oracle's
    distances from the double one in the metrics of the GPU test."""
    c = edge_case(k)
    r = SimpleNamespace()
    for tag, opt in (("one", c.one_step), ("five", c.five)):
        for dt in ("f64", "f32"):
            setattr(r, f"{tag}_{dt}", orc.solve_batch(c.rig, c.cons, c.th0, opt, enabled=c.enabled, dtype=dt))
    r.step32 = step_distance(r.one_f32["theta"], r.one_f64["theta"], c.th0)
    r.err0_32 = err0_distance(r.one_f32["error_history"], r.one_f64["error_history"])
    r.solve32 = solve_distance(r.five_f32["theta"], r.five_f64["theta"])
    return r


def test_grid_is_what_it_says():
    assert NUM_CASES == 72
    seen = set()
    for k in range(NUM_CASES):
        c = edge_case(k)
        assert grid_index(c.J, c.shape, (c.n, c.Kp, c.Ko)) == k
        seen.add((c.J, c.shape, c.n, c.U))
        assert c.rig.num_joints == c.J and c.cons.Kp == c.Kp and c.cons.Ko == c.Ko
        assert c.U == c.Kp + 3 * c.Ko == {1: 1, 15: 64, 31: 191, 32: 192}.get(c.n, c.U) and c.U <= 192
        assert int(c.enabled.sum()) == c.n
        assert c.J - 1 in c.cons.pos_parent
        # every enabled column is live for every instance: the solved count after the structural-zero elimination is n
        for b in range(BATCH):
            Jm, _, _ = orc.eval_jacobian(c.rig, c.cons.instance(b), c.th0[b].astype(np.float64) + 0.1, dtype="f64")
            assert np.all(np.abs(Jm[:, c.enabled != 0]).max(axis=0) > 0), (k, b)
        if c.shape == "chain":  # depth J - 1: six pointer-jumping rounds from 33 joints on
            assert np.array_equal(np.asarray(c.rig.parent).reshape(-1), np.arange(-1, c.J - 1))
    assert len(seen) == NUM_CASES
    assert {c[3] for c in seen} == {1, 64, 65, 128, 129, 191, 192} and {c[2] for c in seen} == {1, 15, 16, 17, 31, 32}
    assert sorted({edge_case(k).line_search for k in range(NUM_CASES)}) == [0, 1, 2]
    assert sum(edge_case(k).line_search != 0 for k in range(NUM_CASES)) == NUM_CASES // 3


def test_reference_is_inside_the_caps():
    wide_a, wide_b, redrawn = [], [], []
    for k in range(NUM_CASES):
        c, r = edge_case(k), reference(k)
        for o in (r.one_f64, r.one_f32, r.five_f64, r.five_f32):
            assert np.all(o["status"] == 0), k
        assert np.all(r.one_f64["iterations"] == 1) and np.all(r.five_f64["iterations"] == 5)
        assert np.array_equal(r.five_f32["iterations"], r.five_f64["iterations"])
        h, href = r.five_f32["error_history"], r.five_f64["error_history"]
        assert np.abs(h - href).max() <= 1e-4 * max(1.0, np.abs(href).max()), k
        for th in (r.one_f64["theta"], r.five_f64["theta"]):
            assert np.all(th[:, c.enabled == 0] == c.th0[:, c.enabled == 0])
        assert np.all(np.linalg.norm(r.one_f64["theta"] - c.th0, axis=1) > 1e-3), k  # the step metric's floor is never what divides
        a = r.step32.max() > STEP_BOUND or r.err0_32.max() > ERR0_BOUND
        b = r.solve32.max() > SOLVE_BOUND
        wide_a += [k] if a else []
        wide_b += [k] if b else []
        if c.line_search:  # the replay that decided the draw is the double oracle's own line search
            th, margin = line_search_trace(c.rig, c.cons, c.th0, c.enabled, c.line_search)
            assert margin == c.margin >= DECIDABLE and solve_distance(th, r.five_f64["theta"]).max() <= 1e-12, (k, margin)
        redrawn += [k] if c.redraw else []
        print("case %2d J %2d %-5s n %2d U %3d ls %d redraw %d margin %.1e | float oracle: step %.2e err0 %.2e five %.2e%s%s"
              % (k, c.J, c.shape, c.n, c.U, c.line_search, c.redraw, c.margin, r.step32.max(), r.err0_32.max(), r.solve32.max(),
                 " A" if a else "", " B" if b else ""))  # fmt: skip
    print("float oracle outside the base bounds: (a)", wide_a, "(b)", wide_b, "| drawn again for an undecidable line search:", redrawn)
    assert all(edge_case(k).line_search for k in redrawn)
    assert len(wide_a) <= MAX_WIDENED and len(wide_b) <= MAX_WIDENED, (wide_a, wide_b)


def test_one_step_reference_is_the_normal_equation_step():
    """The double oracle's single iteration against plain numpy: d = solve(J^T J + lambda I, J^T r) over the enabled columns."""
    worst = 0.0
    for k in range(0, NUM_CASES, 5):
        c, r = edge_case(k), reference(k)
        cols = np.flatnonzero(c.enabled)
        for b in range(BATCH):
            Jm, res, _ = orc.eval_jacobian(c.rig, c.cons.instance(b), c.th0[b].astype(np.float64), dtype="f64")
            Jc = Jm[:, cols]
            d = np.linalg.solve(Jc.T @ Jc + LAMBDA * np.eye(len(cols)), Jc.T @ res)
            th = c.th0[b].astype(np.float64)
            th[cols] -= d
            worst = max(worst, np.linalg.norm(th - r.one_f64["theta"][b]) / max(np.linalg.norm(d), 1e-3))
    print("double oracle against the numpy step: %.2e" % worst)
    assert worst <= 1e-7


@functools.lru_cache(maxsize=None)
def per_instance_case(name):
    """Inputs of the per-instance pre-rotation test: B = 16 elements, per-element bone lengths (0.8 .. 1.2 of the rig's) and
    pre-rotations (a random rotation of up to 0.2 rad composed onto the rig's own, unit quaternions in float32), on the 24-joint
    chain with test_per_instance_rigs' options and on a random bushy rig of 40 joints in the fuzz test's regime."""
    B = 16
    if name == "chain24":
        rig = make_test_character(24)
        jj = np.arange(rig.num_joints, dtype=np.int32)
        cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3)
        en = None
        opt = GnOptions.make(min_iterations=10, max_iterations=10, threshold=1.0, regularization=0.05)
    else:
        r0 = np.random.default_rng(4040)
        rig = random_rig(r0, 40, "bushy")
        J = rig.num_joints
        pp = r0.integers(0, J, size=8).astype(np.int32)
        op = r0.integers(0, J, size=5).astype(np.int32)
        pp[0] = J - 1
        cons, th0, _ = make_problem(rig, pp, op, B, seed=4040, perturb=0.25, random_offsets=True, weights="random")
        en = pick_enabled(rig, cons, th0, 32)
        opt = GnOptions.make(min_iterations=5, max_iterations=5, regularization=LAMBDA)
    J = rig.num_joints
    rng = np.random.default_rng(77)
    off = (rig.translation_offset[None] * rng.uniform(0.8, 1.2, size=(B, J, 1))).astype(np.float32)
    pre = np.zeros((B, J, 4), np.float64)
    for b in range(B):
        for j in range(J):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            ang = rng.uniform(-0.2, 0.2)
            pre[b, j] = quat_mul(rig.pre_rotation[j].astype(np.float64), np.array([*(np.sin(ang / 2) * ax), np.cos(ang / 2)]))
    pre /= np.linalg.norm(pre, axis=2, keepdims=True)
    return SimpleNamespace(rig=rig, cons=cons, th0=th0, enabled=en, opt=opt, off=off, pre=pre.astype(np.float32))


def test_per_instance_inputs_are_fair():
    """Unit quaternions in float32 that differ from the rig's, and the float oracle inside the GPU test's 1e-5 on every element."""
    import copy

    for name in ("chain24", "bushy40"):
        p = per_instance_case(name)
        assert np.abs(np.linalg.norm(p.pre.astype(np.float64), axis=2) - 1.0).max() <= 1e-6
        assert np.abs(p.pre - p.rig.pre_rotation[None]).max() > 1e-2
        for off in (None, p.off):
            worst = 0.0
            for b in range(p.th0.shape[0]):
                rb = copy.deepcopy(p.rig)
                rb.pre_rotation[:] = p.pre[b]
                if off is not None:
                    rb.translation_offset[:] = off[b]
                r64 = orc.solve(rb, p.cons.instance(b), p.th0[b], p.opt, enabled=p.enabled, dtype="f64")
                r32 = orc.solve(rb, p.cons.instance(b), p.th0[b], p.opt, enabled=p.enabled, dtype="f32")
                assert r64["status"] == 0 and r32["status"] == 0 and r32["iterations"] == r64["iterations"]
                worst = max(worst, np.linalg.norm(r32["theta"] - r64["theta"]) / max(np.linalg.norm(r64["theta"]), 1e-3))
            print("%s %s: float oracle worst %.3e" % (name, "offsets + pre-rotations" if off is not None else "pre-rotations", worst))
            assert worst <= 1e-5
