"""Shapes for the explicit-Jacobian route's kernel forms (momentum_amd/csrc/mmx_kernels.hip), shared by
tests/test_explicit_route_forms_host.py and tests/test_gpu_explicit_route_forms.py.

ne_form and step_form restate the two host dispatchers.  They LABEL the cases and guard their coverage; nothing about a
kernel's result is taken from them.  The rig is the 812-parameter one of tests/test_gpu_many_parameters.py with a
constraint on every joint, so mmx_problem_set_enabled chooses the solved size n and the constraint count chooses M
modulo 4, 16 and 32."""
from __future__ import annotations

import functools

import numpy as np

from momentum_amd import make_rig300
from momentum_amd._abi import MMX_STEP_LM_SCHEDULE, GnOptions
from momentum_amd.rigs import RX, RZ, _build_rig
from tests.helpers import make_problem

LDS_64K, LDS_160K = 64 * 1024, 160 * 1024
K_NE_CHUNK, K_NE_COLS, K_CHUNK_LOADS, K_MAX_SOLVED = 32, 8, 10, 2048  # kNeChunk, kNeCols, kChunkLoads, kMaxSolved
MFMA_TPW = (4, 8, 12, 16, 24, 32, 40, 48)


def ne_form(n: int, M: int):
    """launchNormalEquations (mmx_kernels.hip, `if (pb.n >= 32 && pb.n <= 384)` ... `MMX_NE_LAUNCH(48)`, then the
    normalEquationsKernel launch) with normalEquationsChunkRows and the pass loop of normalEquationsMfmaKernel
    (`for (int base = 0; base < T; base += 4 * TPW)`).  J is the library's own 256-byte aligned scratch, so kVec is
    M % 4 == 0.  ("valu", chunk) | ("mfma", TPW, vec, passes)."""
    assert 1 <= n <= K_MAX_SOLVED
    if 32 <= n <= 384:
        NB = (n + 15) >> 4
        T = NB * (NB + 1) // 2
        need = (T + 3) // 4
        tpw = next((t for t in MFMA_TPW[:-1] if need <= t), MFMA_TPW[-1])
        return ("mfma", tpw, M % 4 == 0, -(-T // (4 * tpw)))
    nT = (n + 3) >> 2
    return ("valu", K_NE_CHUNK if K_NE_CHUNK * (4 * nT + 5) * 4 <= LDS_160K - 64 else K_NE_CHUNK // 2)


def cholesky_step_lds_bytes(n: int, M: int) -> int:
    """choleskyStepLdsBytes (mmx_kernels.hip)."""
    return (n * ((n + 1) | 1) + 3 * n + M + 12) * 4


def _tiled_lds_bytes(n: int, chunk_rows: int) -> int:
    """tiledLdsFloats (mmx_kernels.hip) for chunkRows > 0, in bytes."""
    NP = (n + 15) & ~15
    pan = (max(NP * 16, n * (chunk_rows + 1)) + 3) & ~3
    return (pan + 3 * NP + ((chunk_rows + 3) & ~3) + 512 + 8) * 4


def step_form(n: int, M: int):
    """launchCholeskyStep (mmx_kernels.hip, from `size_t lds = choleskyStepLdsBytes(pb.n, pb.M)` to the choleskyStepKernel
    launch); in-place fetch is the loop `for (int base = 256 * kChunkLoads; base < items; ...)` of choleskyStepTiledKernel
    with items = n * chunkRows / 4.  ("lds", over_64k) | ("tiled", kM, chunkRows, inplace_fetch).  The tiled refinement's
    vec4 is M % 4 == 0 (step_vec4): a property of the constraint set, not of n."""
    assert 1 <= n <= K_MAX_SOLVED
    lds = cholesky_step_lds_bytes(n, M)
    if lds <= LDS_160K:
        return ("lds", lds > LDS_64K)
    chunk_rows = 32 if n * 8 <= 256 * K_CHUNK_LOADS else 16
    if _tiled_lds_bytes(n, chunk_rows) > LDS_160K - 64:
        chunk_rows = 8
    assert _tiled_lds_bytes(n, chunk_rows) <= LDS_160K - 64
    return ("tiled", 2 if n <= 512 else K_NE_COLS, chunk_rows, n * chunk_rows // 4 > 256 * K_CHUNK_LOADS)


def step_vec4(M: int) -> bool:
    return M % 4 == 0


# ---- the rig ----------------------------------------------------------------------------------------------------------


def many_parameter_rig(extra_dofs, unit=0.01):
    """make_rig300 (BASELINE configs[4]) with `extra_dofs` rotation parameters on every joint beyond the 72-joint body
    instead of one on 172 of them: 128 + 228 * extra_dofs parameters."""
    base = make_rig300(unit=unit)  # (metres: lambda = 0.05 stays above the factor's damping floor, kFactorDamping x the mean diagonal)
    J0, J = 72, base.num_joints
    trip = []
    for r in range(7 * J0):
        for k in range(base.pt_outer[r], base.pt_outer[r + 1]):
            trip.append((r, int(base.pt_inner[k]), float(base.pt_value[k])))
    names = list(base.param_names[:128])
    assert max(c for _, c, _ in trip) == 127
    for j in range(J0, J):
        for d in [RX, RX + 1, RZ, 0, 1, 2, 6][:extra_dofs]:  # rotations first, then translations, then the scale
            trip.append((j * 7 + d, len(names), 1.0))
            names.append(f"{base.joint_names[j]}_d{d}")
    return _build_rig(base.parent, base.pre_rotation, base.translation_offset, trip, len(names), list(base.joint_names), names)


P812 = 812
B = 3
# name: rows.  M3597 % 4 = 1, % 16 = 13, % 32 = 13.  M3591 % 4 = 3 (% 16 = % 32 = 7) is the residue at which the LAST lane of a
# ragged scalar piece decides (`kk + 3 < M`, `row + 3 < M`): with M % 4 = 1 a piece that straddles M ends after its first lane.
CONSTRAINT_SETS = {"M3600": 3600, "M3597": 3597, "M3591": 3591}
SEEDS = {"M3600": 4100, "M3597": 4200, "M3591": 4300}
FULL_SETS = ("M3600", "M3597")  # the sets that run every solve shape; M3591 runs the first n of each tiled form


@functools.lru_cache(maxsize=None)
def rig812():
    rig = many_parameter_rig(3)
    assert rig.num_params == P812 and rig.num_joints == 300
    return rig


@functools.lru_cache(maxsize=None)
def constraint_set(name: str):
    """(cons [B = 3], theta_star [3, 812]): a position and an orientation constraint on every joint (M3600, the problem812
    shape of tests/test_gpu_many_parameters.py), or the same minus the last position constraint (M3597) or the last three
    (M3591, the deepest joint's position first).  Instance 2 carries
    instance 0's constraints (and theta_star): a kernel that keeps no cross-instance state gives it instance 0's numbers."""
    rig = rig812()
    joints = np.arange(rig.num_joints, dtype=np.int32)
    pos = {"M3600": joints, "M3597": joints[:-1], "M3591": joints[:-3]}[name]
    if name == "M3591":
        # Row 0 is the position of the deepest joint, which 42 parameters move.  A scalar piece that reads one lane past M
        # lands on row 0 of the NEXT parameter's column: behind the root (one non-zero in that row) it would read zeros and
        # compute the right answer.
        parent = np.asarray(rig.parent)
        depth = np.zeros(len(parent), int)
        for j in range(len(parent)):  # (parents precede their children)
            depth[j] = depth[parent[j]] + 1 if parent[j] >= 0 else 0
        deepest = int(depth[pos].argmax())
        pos = np.r_[pos[deepest], np.delete(pos, deepest)].astype(np.int32)
    cons, _, ths = make_problem(rig, pos, joints, B, seed=SEEDS[name], perturb=0.1)
    assert cons.rows == CONSTRAINT_SETS[name]
    for a in (cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_offset, cons.ori_target, cons.ori_weight):
        a[2] = a[0]
    ths[2] = ths[0]
    return cons, ths


@functools.lru_cache(maxsize=None)
def enabled_set(n: int, salt: int = 0) -> np.ndarray:
    """A seeded random subset of n of the 812 parameters as a uint8 mask: not a contiguous range, so the kernels' enabledList
    is a real indirection.  Constraints sit on every joint: no enabled column is structurally zero, the solve's n is n."""
    rng = np.random.default_rng(9000 + n + 10000 * salt)
    idx = np.sort(rng.choice(P812, size=n, replace=False))
    assert n < 2 or idx[-1] - idx[0] > n - 1
    en = np.zeros(P812, np.uint8)
    en[idx] = 1
    en.setflags(write=False)
    return en


# ---- the named shapes -------------------------------------------------------------------------------------------------


def _ne_shapes():
    """n for mmx_eval_normal_equations, from ne_form (the TPW and the passes do not depend on M)."""
    form = {n: ne_form(n, 3600) for n in range(1, 401)}
    mfma = [n for n in form if form[n][0] == "mfma"]
    ns = [1, 3, 31]  # VALU below the matrix-core kernel: n < 4, n % 4 != 0, the last n of the hand-over
    ns.append(mfma[0])  # 32: the first MFMA n, T = 3 tiles
    for tpw in MFMA_TPW:  # one ragged n (n % 16 = 13) in each single-pass band: TPW 4, 8, 12, 16, 24, 32, 40, 48
        band = [n for n in mfma if form[n][1] == tpw and form[n][3] == 1]
        ns.append(band[-1] - 3)
    two = [n for n in mfma if form[n][3] == 2]
    ns.append(two[0])  # 305: the first n of the second pass over J
    ns += [mfma[-1] - 1, mfma[-1]]  # 383 and 384: the last MFMA sizes, ragged and a multiple of 16 (all twelve pieces per thread)
    ns.append(mfma[-1] + 1)  # 385: the first wide VALU n
    assert all(n % 16 != 0 for n in ns[4:12]) and len(set(ns)) == len(ns)
    return tuple(ns)


def _solve_shapes(M: int):
    """n for the pinned solve, from step_form: both sides of every hand-over of launchCholeskyStep up to the in-place fetch --
    LDS under / over 64 KB, LDS / tiled, 320 / 321 (32 / 16 rows), 512 / 513 (kM), 640 / 641 (in-place fetch)."""
    ns = []
    for n in range(2, 701):
        if step_form(n, M) != step_form(n - 1, M):
            ns += [n - 1, n]
    return tuple(ns)


def _first_of_each_tiled_form(M: int):
    ns, seen = [], set()
    for n in _solve_shapes(M):
        f = step_form(n, M)
        if f[0] == "tiled" and f not in seen:
            seen.add(f)
            ns.append(n)
    return tuple(ns)


NE_SHAPES = _ne_shapes()
SOLVE_SHAPES = {name: _solve_shapes(M) if name in FULL_SETS else _first_of_each_tiled_form(M) for name, M in CONSTRAINT_SETS.items()}
NE_CASES = [(name, n) for name in CONSTRAINT_SETS for n in NE_SHAPES]
SOLVE_CASES = [(name, n) for name in CONSTRAINT_SETS for n in SOLVE_SHAPES[name]]


def _deferred_shapes():
    """One n per step form on M3597, for the solves that put stepUpdateKernel behind the step: the in-LDS step (above 64 KB),
    tiled <2> with 32 and with 16 rows, tiled <kNeCols> (16 rows, in-place fetch)."""
    M = CONSTRAINT_SETS["M3597"]
    want = [("lds", True), ("tiled", 2, 32, False), ("tiled", 2, 16, False), ("tiled", K_NE_COLS, 16, True)]
    ns = SOLVE_SHAPES["M3597"]
    return tuple(next(n for n in ns if step_form(n, M) == f) for f in want)


DEFERRED_SHAPES = _deferred_shapes()
DEFERRED_RULES = ("line_search_2", "lm_schedule")
DEFERRED_CASES = [(n, rule) for n in DEFERRED_SHAPES for rule in DEFERRED_RULES]


# ---- the solves -------------------------------------------------------------------------------------------------------

# The enabled set of a solve shape: enabled_set(n, salt), salt 0 unless the shape is listed.  The listed shapes are the ones
# whose salt-0 set the oracle's FLOAT solve did not stay inside the solve's bounds on (its error after the first, long step
# is the entry that misses: 1e-4 relative of a number that one unrefined float Cholesky solve of that system does not pin);
# their salt is the first of 0 ... 11 at which it does with room to spare -- at most 0.7 of the history bound and within the
# 1e-5 on the parameters, with every ISA candidate of oracle.py.  Chosen on the CPU before any GPU run
# (tests/test_explicit_route_forms_host.py holds the condition); no bound was moved.
SOLVE_SALT = {("M3600", 321): 2, ("M3600", 512): 2, ("M3600", 640): 6, ("M3600", 641): 2, ("M3597", 640): 11, ("M3591", 641): 3}


def solve_enabled(name: str, n: int) -> np.ndarray:
    return enabled_set(n, SOLVE_SALT.get((name, n), 0))


# Element 1 starts at its solution, so the first convergence test it is allowed (min_iterations = 1: after its second error)
# sees a relative change of a few FLT_EPSILON, far below SOLVE_THRESHOLD x FLT_EPSILON, and it sits out the rest; elements 0
# and 2 still gain two orders of magnitude and more per iteration (a relative change above 5e8 x FLT_EPSILON) and take all
# of max_iterations.  tests/test_explicit_route_forms_host.py holds both, for the oracle in float and in double.
#
# At theta_star itself the error of element 1 would be the float rounding of its targets (2.5e-12 in the oracle's double
# run, 1.1e-10 in its float run): no single-precision implementation can be held to an error history made of rounding
# alone.  So element 1 carries a fixed residual -- its disabled parameters sit ELEMENT1_OFFSET off theta_star -- and starts
# at the minimum of THAT problem over the enabled parameters (the oracle's double solve from theta_star, PRESOLVE_ITERATIONS
# Gauss-Newton iterations, rounded to float): its errors are ~1e-1, the same number in either precision.
SOLVE_THRESHOLD = 1e3
ELEMENT1_OFFSET = 0.01
PRESOLVE_ITERATIONS = 6


def solve_options(rule: str = "plain") -> GnOptions:
    if rule == "plain":
        return GnOptions.make(min_iterations=1, max_iterations=3, threshold=SOLVE_THRESHOLD, regularization=0.05)
    if rule == "line_search_2":
        return GnOptions.make(min_iterations=1, max_iterations=4, threshold=SOLVE_THRESHOLD, regularization=0.05, do_line_search=2)
    assert rule == "lm_schedule"
    return GnOptions.make(min_iterations=1, max_iterations=4, threshold=SOLVE_THRESHOLD, regularization=0.05, step_rule=MMX_STEP_LM_SCHEDULE)


@functools.lru_cache(maxsize=None)
def solve_start(name: str, n: int) -> np.ndarray:
    """theta0 [3, 812] float32.  Elements 0 and 2: theta_star on every disabled parameter (the targets stay reachable, the
    solve carries no large fixed residual); on the enabled ones zero for element 0 and a seeded start of its own for element 2
    (instance 0's targets from elsewhere).  Element 1 starts at its solution (see SOLVE_THRESHOLD): it is done after its
    first convergence test, so every kernel's `done` gate runs."""
    from oracle import oracle as orc

    orc.build()
    cons, ths = constraint_set(name)
    en = solve_enabled(name, n).astype(bool)
    rng = np.random.default_rng(7000 + n)
    th0 = ths.astype(np.float32).copy()
    th0[0, en] = 0.0
    th0[2, en] = rng.uniform(-0.05, 0.05, size=int(en.sum())).astype(np.float32)
    th0[1, ~en] += (ELEMENT1_OFFSET * rng.uniform(-1, 1, size=int((~en).sum()))).astype(np.float32)
    opt = GnOptions.make(min_iterations=PRESOLVE_ITERATIONS, max_iterations=PRESOLVE_ITERATIONS, threshold=1.0, regularization=0.05)
    th0[1] = orc.solve(rig812(), cons.instance(1), th0[1].astype(np.float64), opt, enabled=solve_enabled(name, n), dtype="f64")["theta"].astype(np.float32)
    th0.setflags(write=False)
    return th0


@functools.lru_cache(maxsize=None)
def oracle_solve(name: str, n: int, rule: str, dtype: str):
    """The oracle's solve of a shape (computed once per process and left unchanged)."""
    from oracle import oracle as orc

    orc.build()
    cons, _ = constraint_set(name)
    return orc.solve_batch(
        rig812(), cons, solve_start(name, n), solve_options(rule), enabled=solve_enabled(name, n), dtype=dtype, nthreads=B,
        step_history=rule == "lm_schedule",
    )  # fmt: skip


def theta_distance(theta, ref_theta) -> np.ndarray:
    """Relative distance per instance, as tests/test_gpu_many_parameters.py measures it."""
    ref_theta = np.asarray(ref_theta, np.float64)
    return np.linalg.norm(np.asarray(theta, np.float64) - ref_theta, axis=1) / np.linalg.norm(ref_theta, axis=1)


def history_within_bound(h, href) -> np.ndarray:
    """The error-history rule of tests/test_gpu_many_parameters.py."""
    return np.abs(h - href) <= 1e-4 * np.abs(href) + 1e-7 * href[:, :1]
