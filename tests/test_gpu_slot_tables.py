"""The one-launch solve's slot tables (phase E writes them, the matrix-core pass and the term records of phase G read them)
at the edges of their layout, and the panel pass of its factorisation: small random trees with shared parameters whose
solved-parameter count, number of extra sources and term-record load are CHOSEN (n = 15 / 16 / 17 / 33: a full block, a lone
column in a second / third block; 0, 1, 17 and more extra sources behind the primary slots; a record loop of more than one
trip; entries split into partial cells), H and g against the oracle; then every instantiation that reads the tables (plain
Gauss-Newton, LM schedule, line search, a plane block, trust region, mixed precision) once against the oracle's solve; then
the guarded re-run of a panel on the rank-deficient chain at lambda = 1e-7.

Bounds: tests/test_gpu_parity.py::test_fused_kernel_normal_equations_match_oracle (2e-5 of the largest entry) for H and g,
tests/test_gpu_fuzz.py::test_random_rig_matches_oracle (2e-5 relative on theta, or three times what the oracle's own float
instantiation loses on the instance) for the solves, tests/test_gpu_weak_damping.py (finite parameters) for the chain."""
import numpy as np
import pytest

from momentum_amd import _abi, capi, make_test_character
from momentum_amd._abi import MMX_PRECISION_MIXED, MMX_STEP_LM_SCHEDULE, MMX_STEP_TRUST_REGION, GnOptions
from momentum_amd.rigs import _build_rig
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu

B = 8


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m gpu on the MI355X box)")
    return torch


def slot_rig(seed, J, shared, n, chainy=0.5):
    """A random tree of J joints, every joint constrained.  Every rotation dof of the joints 1 .. J-1 is driven by exactly one
    parameter (J then has full column rank): `shared[i]` dofs of distinct joints by shared parameter i, each other one by a
    parameter of its own.  Returns (rig, enabled mask with exactly n parameters -- the shared ones first --, sources: per
    parameter the joints it drives)."""
    rng = np.random.default_rng(seed)
    parent = [-1] + [j - 1 if rng.uniform() < chainy else int(rng.integers(max(0, j - 4), j)) for j in range(1, J)]
    pre = np.zeros((J, 4), np.float32)
    for j in range(J):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = rng.uniform(-0.4, 0.4)
        pre[j] = [*(np.sin(ang / 2) * ax), np.cos(ang / 2)]
    off = rng.uniform(-0.3, 0.3, size=(J, 3)).astype(np.float32)
    trip, names, sources = [], [], []

    def new_param(name, joints):
        names.append(name)
        sources.append(list(joints))
        return len(names) - 1

    free = {(j, d) for j in range(1, J) for d in (3, 4, 5)}
    for i, m in enumerate(shared):
        joints = [int(j) for j in rng.permutation(np.arange(1, J))]
        picked = []
        for j in joints:
            dofs = [d for d in (3, 4, 5) if (j, d) in free]
            if dofs and len(picked) < m:
                picked.append((j, int(rng.choice(dofs))))
                free.discard(picked[-1])
        assert len(picked) == m
        p = new_param(f"shared{i}", [j for j, _ in picked])
        for j, d in picked:
            trip.append((7 * j + d, p, float(rng.uniform(0.4, 1.0) * rng.choice([-1.0, 1.0]))))
    for d in range(6):
        trip.append((d, new_param(f"root{d}", [0]), 1.0))
    trip.append((6, new_param("scale", [0]), 1.0))
    for j, d in sorted(free):
        trip.append((7 * j + d, new_param(f"j{j}r{d}", [j]), float(rng.uniform(0.5, 1.5))))
    rig = _build_rig(parent, pre, off, trip, len(names), [f"j{j}" for j in range(J)], names)
    assert n <= len(names)
    en = np.zeros(len(names), np.uint8)
    en[:n] = 1
    return rig, en, sources


def term_lower_bounds(rig, en, sources):
    """The term records of tests' premises, restated from mmx_host_tables.cpp::buildTermRuns: an H entry (row >= col) takes one
    term per pair of sources whose joints lie on one root path, except the pair of the two primary sources.  Returns (lower
    bound on all terms, the largest lower bound of one entry, number of extra sources)."""
    J = rig.num_joints
    anc = np.zeros((J, J), bool)  # anc[a, b]: a is b or above it
    for b in range(J):
        a = b
        while a >= 0:
            anc[a, b] = True
            a = int(rig.parent[a])
    rel = anc | anc.T
    cols = [sources[p] for p in np.flatnonzero(en)]
    total, worst = 0, 0
    for r in range(len(cols)):
        for c in range(r + 1):
            if len(cols[r]) == 1 and len(cols[c]) == 1:
                continue  # primary x primary only: the matrix-core pass
            t = int(rel[np.ix_(cols[r], cols[c])].sum()) - 1
            total, worst = total + max(t, 0), max(worst, t)
    return total, worst, sum(len(c) - 1 for c in cols)


def _problem(torch, rig, cons, en, **kw):
    pb = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
    f = lambda a, shp: np.ascontiguousarray(a, np.float32).reshape(shp)
    pb.set_constraints(f(cons.pos_offset, (B, cons.Kp, 3)), f(cons.pos_target, (B, cons.Kp, 3)), f(cons.pos_weight, (B, cons.Kp)),
                       f(cons.ori_offset, (B, cons.Ko, 4)), f(cons.ori_target, (B, cons.Ko, 4)), f(cons.ori_weight, (B, cons.Ko)), **kw)  # fmt: skip
    pb.set_enabled(en)
    pb.set_route("fused")
    return pb


LAYOUTS = {
    # name: (joints, sizes of the shared parameters, n, chain share, premise on (all terms, one entry's terms, extra sources))
    "n15_no_records": (12, [], 15, 0.5, lambda tot, worst, ex: tot == 0 and ex == 0),
    "n16_one_extra": (12, [2], 16, 0.5, lambda tot, worst, ex: ex == 1 and tot >= 1),  # nsrc = 17: no multiple of 16
    "n17_seventeen_extras_split_entries": (22, [18], 17, 0.5, lambda tot, worst, ex: ex == 17 and worst > 8),  # numComb > 0
    "n33_one_extra": (16, [2], 33, 0.5, lambda tot, worst, ex: ex == 1),
    # thirty shared parameters of three sources each on a chain: entries of at most 3 x 3 - 1 = 8 terms (none split), more than
    # 8 x 256 terms in all -- some thread holds more than eight records: termRounds > 8
    "n33_second_trip": (34, [3] * 30, 33, 1.0, lambda tot, worst, ex: ex == 60 and worst <= 8 and tot > 8 * 256),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_normal_equations_at_the_layout_edges(torch_cuda, orc, name):
    torch = torch_cuda
    J, shared, n, chainy, premise = LAYOUTS[name]
    rig, en, sources = slot_rig(100 + len(name), J, shared, n, chainy)
    tot, worst, extras = term_lower_bounds(rig, en, sources)
    assert premise(tot, worst, extras), (name, tot, worst, extras)
    allj = list(range(J))
    cons, th0, _ = make_problem(rig, allj, allj, B, seed=100, perturb=0.4, random_offsets=True, weights="random")
    cons.pos_function_weight, cons.ori_function_weight = 0.8, 1.25
    pb = _problem(torch, rig, cons, en, pos_function_weight=0.8, ori_function_weight=1.25)
    rng = np.random.default_rng(9)
    theta = rng.uniform(-0.4, 0.4, size=(B, rig.num_params)).astype(np.float32)
    lst, jtj, jtr = pb.fused_normal_equations(torch.from_numpy(theta).to(pb.device))
    jtj, jtr = jtj.cpu().numpy(), jtr.cpu().numpy()
    assert len(lst) == n and np.array_equal(np.sort(lst), np.flatnonzero(en))
    for b in range(B):
        Jo, r, _ = orc.eval_jacobian(rig, cons.instance(b), theta[b].astype(np.float64), enabled=en, dtype="f64")
        H = Jo[:, lst].T @ Jo[:, lst]
        g = Jo[:, lst].T @ r
        eh, eg = np.abs(jtj[b] - H).max() / max(1.0, np.abs(H).max()), np.abs(jtr[b] - g).max() / max(1.0, np.abs(g).max())
        print(f"{name} b={b}: H {eh:.2e}  g {eg:.2e}  (terms >= {tot}, one entry >= {worst}, extras {extras})")
        assert eh <= 2e-5, (name, b)
        assert eg <= 2e-5, (name, b)
        assert np.array_equal(jtj[b], jtj[b].T)


@pytest.fixture(scope="module")
def solve_case(orc):
    """One rig for every instantiation: n = 33 (three blocks, a lone column in the third), one shared parameter with 18
    sources (extras past a 16-slot pad, split entries) and one with 3."""
    rig, en, sources = slot_rig(4242, 22, [18, 3], 33, 0.5)
    tot, worst, extras = term_lower_bounds(rig, en, sources)
    assert extras == 19 and worst > 8
    allj = list(range(rig.num_joints))
    cons, th0, _ = make_problem(rig, allj, allj, B, seed=7, perturb=0.25, random_offsets=True, weights="random")
    return rig, en, cons, th0


INSTANTIATIONS = {
    "plain": dict(regularization=0.5),
    "lm_schedule": dict(regularization=0.5, step_rule=MMX_STEP_LM_SCHEDULE),
    "line_search": dict(regularization=0.5, do_line_search=2),
    "plane_block": dict(regularization=0.5),
    "trust_region": dict(step_rule=MMX_STEP_TRUST_REGION),
    "mixed": dict(regularization=0.5, precision=MMX_PRECISION_MIXED),
}


@pytest.mark.parametrize("name", list(INSTANTIATIONS))
def test_solve_parity_across_instantiations(torch_cuda, orc, solve_case, name):
    from tests.test_oracle_joint_blocks import make_block

    torch = torch_cuda
    rig, en, cons, th0 = solve_case
    kw, full = {}, cons
    if name == "plane_block":
        blocks = [make_block(_abi.MMX_JC_PLANE, np.array([3, 9, 14], np.int32), np.random.default_rng(3), weight=1.0, batch=B)]
        kw = dict(joint_blocks=blocks)
        full = orc.Constraints(cons.pos_parent, cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_parent, cons.ori_offset,
                               cons.ori_target, cons.ori_weight, joint_blocks=blocks)  # fmt: skip
    pb = _problem(torch, rig, cons, en, **kw)
    opt = GnOptions.make(min_iterations=5, max_iterations=5, threshold=1.0, **INSTANTIATIONS[name])
    out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt, want_history=True)
    assert pb.last_route() == "fused"
    ref = orc.solve_batch(rig, full, th0, opt, enabled=en, dtype="f64")
    th = out["theta"].cpu().numpy()
    den = np.maximum(np.linalg.norm(ref["theta"], axis=1), 1e-3)
    rel = np.linalg.norm(th - ref["theta"], axis=1) / den
    ref32 = orc.solve_batch(rig, full, th0, opt, enabled=en, dtype="f32")
    tol = np.maximum(2e-5, 3.0 * np.linalg.norm(ref32["theta"] - ref["theta"], axis=1) / den)
    print(f"{name}: rel {rel.max():.2e}  tol {tol.min():.2e}")
    assert np.all(rel <= tol), (name, rel, tol)
    assert np.array_equal(out["iterations"].cpu().numpy(), ref["iterations"])
    assert np.array_equal(out["status"].cpu().numpy() & 3, ref["status"])
    h, href = out["error_history"].cpu().numpy(), ref["error_history"]
    assert np.abs(h - href).max() <= 1e-4 * max(1.0, np.abs(href).max())
    assert np.all(th[:, en == 0] == th0[:, en == 0])


def test_guarded_panel_on_the_weakly_damped_chain(torch_cuda):
    """BASELINE configs[0]'s shape (24-joint chain, three position constraints: nine rows for 31 parameters) at lambda = 1e-7:
    pivots at rounding level, the panel that fails its check is reloaded and eliminated again with the guard.  Finite
    parameters (tests/test_gpu_weak_damping.py: whatever the damping, a step is always taken, never a non-finite one), no
    MMX_SOLVE_NONFINITE, and two solves agree bit for bit."""
    torch = torch_cuda
    rig = make_test_character(24)
    cons, th0, _ = make_problem(rig, [23, 12, 5], [], B, seed=777, perturb=0.3)
    pb = _problem(torch, rig, cons, np.ones(rig.num_params, np.uint8))
    opt = GnOptions.make(min_iterations=10, max_iterations=10, threshold=1.0, regularization=1e-7)
    outs = []
    for _ in range(2):
        out = pb.solve(torch.from_numpy(th0.copy()).to(pb.device), opt, want_history=True)
        assert pb.last_route() == "fused"
        outs.append({k: out[k].cpu().numpy() for k in ("theta", "error", "iterations", "status", "error_history")})
    a, b = outs
    assert np.isfinite(a["theta"]).all()
    assert np.all(a["status"] & _abi.MMX_SOLVE_NONFINITE == 0)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
