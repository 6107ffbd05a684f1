#!/usr/bin/env python3
"""bench.py -- character IK solves/sec on MI355X (BASELINE.json metric) + J-assembly HBM roofline.

    python bench.py --gpus N --steps K --warmup W [--batch B] [--config cfg2|cfg2_all|cfg3|cfg5|cfg2_tracker|...]
                    [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch: a full batched solve (10 Gauss-Newton
iterations: FK -> Jacobian/residual -> JtJ/Jtr -> Cholesky (+1 refinement) -> theta update) of
B independent 72-joint humanoid instances per GPU, inputs resident in HBM.  For N > 1 the driver
launches one rank per GPU (torch.distributed.run); instances are sharded (weak scaling: B per GPU
fixed) and the only collective is one all-reduce of the per-batch residual norms per solve.

A plain run sets up the seeded batch, runs W untimed and K timed steps and prints ONE JSON line on rank 0:
metric/value/unit/higher_is_better/dtype/ms_per_step/... and "check" with the reduced residual norms of the last
step.  --dump-outputs DIR writes what the last timed step returned (rank 0's shard) as DIR/<name>.npy: theta, error,
iterations, status (float32 / float64; a fixed, seeded sample of instances when they would exceed 64 MB, its indices
in DIR/instances.npy) and the reduced norms; the inputs are the same from run to run.
--full adds everything else, each part outside the timed region:
  "check":          parity of THIS batch: the first --check-instances (default 1024) DISTINCT instances of
                    the timed batch re-solved by the CPU oracle in double precision; max / median
                    relative pose-parameter difference (north_star bound: 1e-5)
  "roofline":       achieved algorithmic HBM GB/s of the J-assembly kernel (mmx_eval_jacobian),
                    timed live with HIP events on the launch stream
  "roofline_fused": the headline kernel (fusedSolveKernel): dense-equivalent TFLOP/s of the timed solve
                    and its PMC utilisation figures from the committed profile
  "cpu_baseline":   the CPU oracle (restatement of momentum's algorithm, kind "port") timed on
                    this box's host cores on a bounded sample of the SAME instances
  "configs":        (N = 1 only) every other BASELINE.json configuration that fits one GPU -- the north-star
                    target 65536 x 72 (cfg3, LM schedule), the weak-scaling shard 32768 x 72, the wide-J
                    300-joint rig (cfg5), the batched driver's default line search, a tracker-shaped problem (cfg2 +
                    plane block + parameter limits) -- each with its own solves/s, cpu_baseline and parity check
  and the details file (--details)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X datasheet (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)
FP32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32 vector = fp32-input MFMA peak
UNIT = 0.01  # rig offsets "U[2,30] cm" expressed in metres
PARITY_BOUND = 1e-5  # BASELINE.json north_star: relative difference on pose parameters

CONFIGS = {
    # name: (rig variant, constraint joints, default batch per GPU, step rule, description)
    "cfg2": ("p128", "landmarks", 4096, 0, "BASELINE configs[1]: B x 72-joint humanoid (P=128), position+orientation on 16 landmark joints (M=192), GN lambda=0.05, 10 iterations"),
    "cfg3": ("p128", "landmarks", 65536, 1, "BASELINE configs[2]: 65536 x 72-joint humanoid (P=128, M=192), LM gain-ratio damping schedule (lambda0=0.05), 10 iterations"),
    "cfg4": ("p128", "landmarks", 32768, 0, "BASELINE configs[3]: 262144 x 72-joint humanoid over 8 GPUs = 32768 per GPU (P=128, M=192), GN lambda=0.05, 10 iterations (weak scaling: the per-GPU shard of cfg2's problem)"),
    "cfg5": ("rig300", "cfg5", 8192, 0, "BASELINE configs[4]: 8192 x 300-joint hand+body rig (P=300), 150 position + 50 orientation constraints (M=900), GN lambda=0.05, 10 iterations"),
    "cfg2_all": ("p219", "all", 4096, 0, "BASELINE configs[1] stress variant: P=219, position+orientation on all 72 joints (M=864)"),
    "cfg2_p219": ("p219", "landmarks", 4096, 0, "P=219 parameter set, position+orientation on the 16 landmark joints (route selection probe)"),
    "cfg2_half": ("p219", "half", 4096, 0, "P=219 parameter set, position+orientation on every other joint (route selection probe)"),
    # production-shaped: what marker_tracker.cpp:916-960 adds to the marker constraints -- a plane block (8 floor contacts,
    # PlaneErrorFunction) and MinMax limits on 16 parameters (LimitErrorFunction); takes the fused solve's general rows
    "cfg2_tracker": ("p128", "landmarks+tracker", 4096, 0, "BASELINE configs[1] + PlaneErrorFunction (8 constraints) + 16 MinMax parameter limits (M=192+8+16)"),
    # the reference's own asset: examples/convert_model/test_data/character_with_motion.glb (skeleton + parameter transform read from
    # the FB_momentum extension by momentum_amd.model_io; the committed fixture tests/golden/real_rig_character_with_motion.npz
    # carries what the loader extracted -- the GPU box has no reference checkout), constraints as momentum/test/character_solver/
    # solver_test.cpp:90-103 places them: position + orientation on every joint
    "glb": ("fixture:real_rig_character_with_motion.npz", "all", 4096, 0, "the reference's character_with_motion.glb (3 joints, 10 parameters), position+orientation on every joint (M=36)"),
}

# pymomentum's batched driver as it is called without arguments (pymomentum/tensor_ik/solver_options.h:28-37: lambda = 0.01, at least 4
# and at most 50 iterations, threshold 10, line search on -- the rule of the solvers it selects, SubsetGN / GN-QR): a
# convergence-driven exit per element instead of BASELINE's ten fixed iterations
DRIVER_DEFAULTS = dict(regularization=0.01, min_iterations=4, max_iterations=50, threshold=10.0, do_line_search=2)

# what the default single-GPU run reports besides the headline: (key, config, batch, line_search, timed steps, CPU sample, lambda[, dtype])
EXTRA_RUNS = [
    ("cfg3@65536", "cfg3", 65536, 0, 4, 8192, 0.05),
    ("cfg2@32768", "cfg2", 32768, 0, 6, 8192, 0.05),
    ("cfg2@4096 line_search=2", "cfg2", 4096, 2, 10, 4096, 0.05),
    ("cfg5@8192", "cfg5", 8192, 0, 3, 1024, 0.05),
    # SURVEY 8(d)'s stress variant (the shape of solver_test.cpp:90-103): P = 219, both constraints on all 72 joints, M = 864
    ("cfg2_all@4096", "cfg2_all", 4096, 0, 4, 1024, 0.05),
    ("cfg2_tracker@4096", "cfg2_tracker", 4096, 0, 10, 4096, 0.05),
    # the batched driver's real defaults (DRIVER_DEFAULTS): what a solve_ik caller sees, on BASELINE's rig and on the reference's own
    ("cfg2@4096 solve_ik defaults", "cfg2", 4096, 2, 6, 1024, 0.01, "f32", 0, True),
    ("glb@4096 solve_ik defaults", "glb", 4096, 2, 6, 2048, 0.01, "f32", 0, True),
    # MMX_PRECISION_MIXED (ABI 11): double theta / FK / residuals / g / linear-solve residual around the single-precision factor
    # (with the batched driver's line search, like the AUTO line below: without one the undamped iteration is chaotic in double on a
    # few per cent of these instances -- profiles/r06_weak_damping.json has both)
    ("cfg2@4096 lambda=1e-3 line_search=2 precision=mixed", "cfg2", 4096, 2, 6, 1024, 1e-3, "f32", 3),
    ("cfg3@65536 precision=mixed", "cfg3", 65536, 0, 3, 4096, 0.05, "f32", 3),
    # the double instantiation (mmx_solve_f64, SolverT<double>) on the weak-damping case the single-precision line below
    # cannot hold: checked against the oracle's double run on the instances whose line-search decisions agree, with the
    # oracle's DOUBLE instantiation as its CPU baseline
    ("cfg2@4096 lambda=1e-5 line_search=2 dtype=f64", "cfg2", 4096, 2, 3, 1024, 1e-5, "f64"),
    # MMX_PRECISION_AUTO at a damping where single precision loses the bound on part of the batch (profiles/r05_weak_damping.json):
    # single precision first, the elements its precision estimate marks re-solved in double on the same stream (with the batched
    # driver's line search: without one the undamped iteration is chaotic in double on a few per cent of these instances)
    ("cfg2@4096 lambda=1e-3 line_search=2 precision=auto", "cfg2", 4096, 2, 6, 2048, 1e-3, "f32", 2),
    # weak damping (pymomentum's test_solver2.py value) with the batched driver's line search: on this shape -- as many
    # independent rows as solved parameters -- no single-precision Cholesky solver holds 1e-5 on theta (check.pass is
    # false by construction, the float oracle's figures stand beside it); tests/test_gpu_weak_damping.py has the table
    ("cfg2@4096 lambda=1e-5 line_search=2", "cfg2", 4096, 2, 10, 2048, 1e-5),
]


def algorithmic_bytes_per_instance(M: int, P: int, Kp: int, Ko: int) -> int:
    """write J (M*P) and r (M), read theta (P), constraint payload and
    parent indices; fp32; rig constants are batch-shared and excluded."""
    return 4 * (M * P + M) + 4 * P + 4 * (7 * Kp + 9 * Ko) + 4 * (Kp + Ko)


def dense_equivalent_flops_per_iteration(M: int, n: int, J: int) -> float:
    """what a dense implementation of one GN iteration executes per instance --
    J^T J (lower triangle, M n^2 MACs = 2 flops each, half of it by symmetry), J^T r, Cholesky n^3/3,
    two triangular solves, FK.  The fused kernel never forms J and exploits the tree sparsity, so it
    executes far fewer; this is the denominator a dense GPU/CPU implementation would be priced against."""
    return float(M) * n * n + 2.0 * M * n + n**3 / 3.0 + 2.0 * n * n + 150.0 * J


def build_rig(config: str):
    from momentum_amd import humanoid72_landmark_joints, make_humanoid72

    variant, which, defB, step_rule, desc = CONFIGS[config]
    if variant.startswith("fixture:"):
        from momentum_amd.rigs import Rig

        g = np.load(os.path.join(ROOT, "tests", "golden", variant.split(":", 1)[1]))
        rig = Rig(g["parent"], g["pre_rotation"], g["translation_offset"], g["pt_outer"], g["pt_inner"], g["pt_value"], g["pt_offsets"],
                  len(g["param_names"]), [str(x) for x in g["joint_names"]], [str(x) for x in g["param_names"]])  # fmt: skip
        allj = np.arange(rig.num_joints, dtype=np.int32)
        return rig, (allj, allj), defB, step_rule, desc
    if variant == "rig300":
        from momentum_amd import make_rig300

        rig = make_rig300(seed=12345, unit=UNIT)
    else:
        rig = make_humanoid72(seed=12345, variant=variant, unit=UNIT)
    if which.startswith("landmarks"):
        pos_parents = ori_parents = humanoid72_landmark_joints(rig)
    elif which == "cfg5":
        prng = np.random.default_rng(77)
        pos_parents = prng.choice(rig.num_joints, size=150, replace=False).astype(np.int32)
        ori_parents = prng.choice(rig.num_joints, size=50, replace=False).astype(np.int32)
    elif which == "half":
        pos_parents = ori_parents = np.arange(0, rig.num_joints, 2, dtype=np.int32)
    else:
        pos_parents = ori_parents = np.arange(rig.num_joints, dtype=np.int32)
    return rig, (np.asarray(pos_parents, np.int32), np.asarray(ori_parents, np.int32)), defB, step_rule, desc


class DeviceBatch:
    """Synthetic batch generated ON the GPU: theta* = U[-0.3,0.3]^P, targets = FK(theta*) through the
    product's own FK kernel, theta0 = 0.  Every instance is distinct."""

    def __init__(self, rig, parents, B, device_index, seed, tracker=False):
        from momentum_amd import _abi, capi

        self.rig, self.parents, self.B = rig, parents, B
        self.last_status, self.last_elapsed_rank = None, None  # of the last solve_loop on this batch
        pos_parents, ori_parents = parents
        self.rh = capi.RigHandle(rig, device_index)
        self.pb = pb = capi.Problem(self.rh, B, pos_parents, ori_parents)
        dev = pb.device
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        P, Kp, Ko = rig.num_params, len(pos_parents), len(ori_parents)
        self.theta_star = (torch.rand((B, P), generator=g, device=dev, dtype=torch.float32) * 2 - 1) * 0.3
        st = pb.skeleton_state(self.theta_star)  # [B,J,8]
        pidx = torch.as_tensor(np.asarray(pos_parents, dtype=np.int64), device=dev)
        oidx = torch.as_tensor(np.asarray(ori_parents, dtype=np.int64), device=dev)
        self.pos_offset = torch.zeros((B, Kp, 3), device=dev)
        self.pos_target = st[:, pidx, 0:3].contiguous()
        self.ori_offset = torch.zeros((B, Ko, 4), device=dev)
        self.ori_offset[..., 3] = 1.0
        self.ori_target = st[:, oidx, 3:7].contiguous()
        self.pos_weight = torch.ones((B, Kp), device=dev)
        self.ori_weight = torch.ones((B, Ko), device=dev)
        self.blocks, self.limits = [], []
        if tracker:
            # planes through the solution's joint positions (random unit normals), MinMax limits that the solution respects
            pj = np.asarray(pos_parents[:8], np.int32)
            nrm = torch.randn((B, len(pj), 3), generator=g, device=dev, dtype=torch.float32)
            nrm = nrm / nrm.norm(dim=-1, keepdim=True)
            pstar = st[:, torch.as_tensor(pj.astype(np.int64), device=dev), 0:3]
            d = (nrm * pstar).sum(-1).contiguous()
            self.blocks = [_abi.JointBlock(_abi.MMX_JC_PLANE, pj, torch.ones((B, len(pj)), device=dev), nrm.contiguous(),
                                           local_point=torch.zeros((B, len(pj), 3), device=dev), plane_d=d)]  # fmt: skip
            self.limits = [_abi.ParameterLimit.minmax(int(p), -0.35, 0.35, 1.0) for p in range(6, 22)]
        pb.set_constraints(self.pos_offset, self.pos_target, self.pos_weight, self.ori_offset, self.ori_target, self.ori_weight, 1.0, 1.0,
                           joint_blocks=self.blocks or None, limits=self.limits or None)  # fmt: skip
        self.theta0 = torch.zeros((B, P), device=dev, dtype=torch.float32)

    def host_constraints(self, n):
        """The first n instances of this very batch as the oracle's input (host copies)."""
        from oracle import oracle as orc

        from momentum_amd import _abi

        c = lambda t: t[:n].cpu().numpy()
        blocks = [_abi.JointBlock(k.type, k.parent, c(k.weight), c(k.global_), c(k.local_point), None, c(k.plane_d), k.function_weight, k.loss)
                  for k in self.blocks]  # fmt: skip
        return orc.Constraints(
            self.parents[0], c(self.pos_offset), c(self.pos_target), c(self.pos_weight),
            self.parents[1], c(self.ori_offset), c(self.ori_target), c(self.ori_weight),
            joint_blocks=blocks, limits=list(self.limits),
        )  # fmt: skip


def make_device_problem(rig, parents, B, device_index, seed):
    """(kept for scripts/): rig handle, problem, theta0, theta* of a DeviceBatch."""
    pos_parents, ori_parents = parents if isinstance(parents, tuple) else (parents, parents)
    db = DeviceBatch(rig, (np.asarray(pos_parents, np.int32), np.asarray(ori_parents, np.int32)), B, device_index, seed)
    make_device_problem.keep = db
    return db.rh, db.pb, db.theta0, db.theta_star


def usable_cores() -> int:
    """Host cores this process may actually use: the affinity mask, capped by the cgroup CPU quota
    (a container can see 256 logical CPUs and be allowed a dozen)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(round(int(quota) / int(period)))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def parity_check(db: DeviceBatch, theta_gpu, options, n, line_search_aware=False):
    """Re-solves the first n (distinct) instances of the timed batch with the CPU oracle in double
    precision and compares the pose parameters (outside the timed region; the oracle is the checker)."""
    from oracle import oracle as orc

    n = int(min(n, db.B))
    if n <= 0:
        return None
    cons = db.host_constraints(n)
    th0 = db.theta0[:n].cpu().numpy()
    ref = orc.solve_batch(db.rig, cons, th0, options, dtype="f64", nthreads=usable_cores())
    th = theta_gpu[:n].cpu().numpy().astype(np.float64)
    rel = np.linalg.norm(th - ref["theta"], axis=1) / np.maximum(np.linalg.norm(ref["theta"], axis=1), 1e-30)
    out = {
        "instances": n,
        "distinct": True,
        "reference": "CPU oracle, double precision (oracle/, kind port), same inputs",
        "max_rel_theta_vs_oracle_f64": float(rel.max()),
        "median_rel_theta_vs_oracle_f64": float(np.median(rel)),
        "p99_rel_theta_vs_oracle_f64": float(np.quantile(rel, 0.99)),
        "num_above_bound": int((rel > PARITY_BOUND).sum()),
        "bound": PARITY_BOUND,
        "pass": bool(rel.max() <= PARITY_BOUND),
    }
    if options.min_iterations != options.max_iterations:
        out["oracle_iterations"] = [int(x) for x in ref["iterations"]]
    if out["num_above_bound"] > 0:
        # `pass` is the strict bound.  Beside it, for the instances above the bound: what the oracle's own FLOAT instantiation
        # (the restatement of the reference's SolverT<float>) loses on them.  Three things put an instance there without any
        # defect of the kernels: the LM schedule's discrete decisions (rho against 0 / 0.25 / 0.75: a gain ratio on a threshold
        # goes the other, equally valid, way in single precision), a Gauss-Newton run that has not converged (no line search,
        # a start from which the undamped step overshoots: the iteration amplifies every last-bit difference), and a weak
        # lambda on a rank-deficient J (tests/test_gpu_weak_damping.py).  pass_relaxed: at least 99 % of the instances within
        # the bound and every instance above it above it in the float oracle too.
        idx = np.nonzero(rel > PARITY_BOUND)[0]
        sub = cons.subset(idx)  # (the same problem: joint blocks / limits / prior travel with the instances)
        with np.errstate(all="ignore"):
            r32 = orc.solve_batch(db.rig, sub, th0[idx], options, dtype="f32", nthreads=usable_cores())
            rel32 = np.linalg.norm(r32["theta"] - ref["theta"][idx], axis=1) / np.maximum(np.linalg.norm(ref["theta"][idx], axis=1), 1e-30)
        out["above_bound_instances"] = [int(i) for i in idx[:16]]
        out["above_bound_rel"] = [float(x) for x in rel[idx][:16]]
        out["above_bound_float_oracle_rel"] = [float(x) for x in rel32[:16]]
        out["above_bound_float_oracle_also_above"] = bool(np.all(~(rel32 <= PARITY_BOUND)))
        out["above_bound_final_error_double"] = [float(x) for x in ref["error"][idx][:16]]
        # ... and whether the double run itself was converging on them.  Plain Gauss-Newton (no line search) from a start where
        # the undamped step overshoots RAISES its error at some iteration, or ends with less than 1e3 of reduction: such a run
        # amplifies every last-bit difference (the reference's own float instantiation ends 1e-3 ... 0.4 from its double one
        # on them, above_bound_float_oracle_rel).  num_above_bound_on_converging_runs counts the instances above the bound
        # whose double run decreased its error at every iteration and by 1e3 overall; above_bound_closer_than_float_oracle
        # says that on every instance above the bound the GPU answer is nearer to the double one than the float oracle's is.
        hist = np.concatenate([ref["error_history"][idx], ref["error"][idx][:, None]], axis=1)
        h0 = hist[:, 0]
        its = np.asarray(ref["iterations"])[idx].astype(int)
        raised = np.array([bool(np.any(np.diff(hist[k, : its[k]]) > 0.0) or hist[k, -1] > hist[k, its[k] - 1]) for k in range(len(idx))])
        diverging = raised | ~(ref["error"][idx] <= 1e-3 * h0)
        out["above_bound_initial_error_double"] = [float(x) for x in h0[:16]]
        out["above_bound_double_run_raised_its_error"] = [bool(x) for x in raised[:16]]
        out["above_bound_closer_than_float_oracle"] = bool(np.all(rel[idx] <= rel32))
        out["num_above_bound_on_converging_runs"] = int((~diverging).sum())
        out["pass_relaxed"] = bool(out["num_above_bound"] <= n // 100 and out["above_bound_float_oracle_also_above"])
        out["pass_relaxed_rule"] = ">= 99 % within the bound; every instance above it is above it in the oracle's float instantiation too"
    out["within_bound"] = f"{n - out['num_above_bound']}/{n}"
    if line_search_aware:
        out["note"] = "backtracking takes discrete decisions: an instance whose accept test sits on its threshold goes the other, equally valid, way in another precision (tests/test_gpu_weak_damping.py separates those by step length); `pass` here is the plain bound on every checked instance"
    return out


def lm_branch_analysis(gpu_steps, gpu_err, ref, rel, bound=PARITY_BOUND):
    """LM schedule (BASELINE configs[2]): the GPU run's DECISIONS against the double oracle's, exactly.  Per iteration the
    schedule decides twice on the gain ratio rho = actual / predicted decrease (the quantity TrustRegionQRT compares with its
    thresholds, momentum/character_solver/trust_region_qr.cpp:244-268): accept iff rho > 0; lambda x lm_up iff not
    rho >= 0.25, x lm_down iff rho > 0.75.  gpu_steps [n][K][2] = (lambda, rho) per iteration from mmx_solve_with_step_history,
    ref = the oracle's double run with step_history.  An instance has the SAME decisions when every iteration's (accept,
    scale class) pair agrees -- its lambda sequence is then the double run's, checked to 1e-6 -- and is held to `bound` on theta.
    Every other instance is a BRANCH FLIP: at its first diverging iteration the two gain ratios lie on opposite sides of a
    threshold; reported with the double run's distance to that threshold and the two ratios' difference."""
    lam_g, rho_g = gpu_steps[..., 0], gpu_steps[..., 1]
    lam_r, rho_r = np.asarray(ref["lambda_history"]), np.asarray(ref["gain_ratio_history"])
    cls = lambda r: np.where(~(r >= 0.25), 0, np.where(r > 0.75, 2, 1))
    same_it = ((rho_g > 0) == (rho_r > 0)) & (cls(rho_g) == cls(rho_r))
    same_it[:, -1] = (rho_g[:, -1] > 0) == (rho_r[:, -1] > 0)  # (the last iteration's scaling of lambda acts on nothing)
    same = same_it.all(axis=1)
    lam_ok = np.all(np.abs(lam_g - lam_r) <= 1e-6 * np.abs(lam_r), axis=1)
    flips = np.flatnonzero(~same)
    first = np.argmax(~same_it[flips], axis=1) if len(flips) else np.zeros(0, int)
    rg, rr = rho_g[flips, first], rho_r[flips, first]
    thr = np.array([0.0, 0.25, 0.75])
    lo, hi = np.minimum(rg, rr), np.maximum(rg, rr)
    straddled = (thr[None, :] >= lo[:, None]) & (thr[None, :] <= hi[:, None])
    dist = np.where(straddled, np.abs(rr[:, None] - thr[None, :]), np.inf).min(axis=1) if len(flips) else np.zeros(0)
    above = rel > bound
    out = {
        "instances": int(len(rel)),
        "same_decisions": int(same.sum()),
        "lm_branch_flips": int(len(flips)),
        "same_decisions_lambda_sequences_equal": bool(lam_ok[same].all()) if same.any() else True,
        "max_rel_same_decisions": float(rel[same].max()) if same.any() else None,
        "num_above_bound": int(above.sum()),
        "num_above_bound_with_same_decisions": int((above & same).sum()),
        "num_above_bound_that_are_branch_flips": int((above & ~same).sum()),
        "flips_double_rho_within_1e-3_of_threshold": int((dist <= 1e-3).sum()),
        "flips_double_rho_within_1e-2_of_threshold": int((dist <= 1e-2).sum()),
        "flip_max_distance_of_double_rho_to_threshold": float(dist.max()) if len(flips) else 0.0,
        "flip_max_abs_rho_difference": float(np.abs(rg - rr).max()) if len(flips) else 0.0,
        # (for the side file: the flips themselves)
        "flip_instances": [int(i) for i in flips[:64]],
        "flip_iteration": [int(i) for i in first[:64]],
        "flip_rho_gpu": [float(x) for x in rg[:64]],
        "flip_rho_double": [float(x) for x in rr[:64]],
        "flip_rel_theta": [float(x) for x in rel[flips][:64]],
        "flip_final_error_gpu_over_double": [float(a / b) if b > 0 else None for a, b in zip(gpu_err[flips, -1][:64], np.asarray(ref["error_history"])[flips, -1][:64])],
    }
    # pass: theta within the bound wherever the decisions are the double run's, and every other instance a genuine threshold
    # case: at its first diverging iteration the double run's gain ratio within 1e-2 of the threshold the two ratios straddle
    # (measured on 16 384 instances of the cfg3 batch: 31 flips, all within 4.7e-3, 23 within 1e-3; the ones further than
    # 1e-3 sit at iterations 8-9 of a converged fit, where e - e_new is a difference at the noise floor of a float error sum;
    # the oracle's own FLOAT instantiation flips on 263 of the same instances, ratios up to 0.12 apart)
    out["pass"] = bool(out["num_above_bound_with_same_decisions"] == 0 and out["same_decisions_lambda_sequences_equal"]
                       and out["flip_max_distance_of_double_rho_to_threshold"] <= 1e-2)
    return out


def cpu_baseline(db: DeviceBatch, sample, options, dtype="f32", dense_flops_per_solve=None):
    """The CPU oracle timed on the host cores (same precision as the GPU run) on the first `sample` instances of the SAME batch.
    Returns (compact, details): the compact part goes into the bench line, the details into the side file."""
    from oracle import oracle as orc

    cores = usable_cores()
    sample = int(min(sample, db.B))
    cons = db.host_constraints(sample)
    th0 = db.theta0[:sample].cpu().numpy()
    warm = min(sample, 2 * cores)
    orc.solve_batch(db.rig, db.host_constraints(warm), th0[:warm], options, dtype=dtype, nthreads=cores)
    t0 = time.perf_counter()
    orc.solve_batch(db.rig, cons, th0, options, dtype=dtype, nthreads=cores)
    dt = time.perf_counter() - t0
    n1 = max(1, min(sample, 32 if db.rig.num_joints > 100 else 64))
    t1 = time.perf_counter()
    orc.solve_batch(db.rig, db.host_constraints(n1), th0[:n1], options, dtype=dtype, nthreads=1)
    dt1 = time.perf_counter() - t1
    compact = {
        "value": sample / dt,
        "unit": "solves/s",
        "cores": cores,
        "cores_total": os.cpu_count(),
        "kind": "port",
        "sample": f"first {sample} instances of the timed batch, {dtype}, one solver per task over {cores} threads",
        "single_thread_value": n1 / dt1,
    }
    if dense_flops_per_solve:
        # dense-equivalent flops of a solve x single-thread solves/s: what one core of the baseline sustains
        compact["gflops_per_thread"] = dense_flops_per_solve * (n1 / dt1) / 1e9
    details = dict(compact, build=orc.build_info(), note="usable cores = affinity mask and cgroup quota; mirrors tensor_ik.cpp:127 (one task per batch element)")
    return compact, details


def solve_loop(db: DeviceBatch, opt, steps, warmup, dist=None, comm=None, dtype="f32"):
    """W untimed + K timed batched solves; returns (elapsed seconds (max over ranks), theta of the last solve,
    reduced norms).  comm: the direct RCCL communicator (momentum_amd.capi.Comm) when there is one."""
    from momentum_amd import capi
    from momentum_amd import distributed as D

    pb, dev, B = db.pb, db.pb.device, db.B
    theta0 = db.theta0 if dtype == "f32" else db.theta0.double()
    theta = theta0.clone()
    outputs = dict(
        error=torch.empty((B,), dtype=torch.float64, device=dev),
        iterations=torch.empty((B,), dtype=torch.int32, device=dev),
        status=torch.empty((B,), dtype=torch.int32, device=dev),
    )
    norms = torch.zeros(3, dtype=torch.float64, device=dev)

    def step():
        theta.copy_(theta0)
        if dtype == "f32":
            pb.solve(theta, opt, outputs=outputs)
        else:
            outputs.update(pb.solve_f64(theta, opt))
        # the path's only exchange: per-batch residual norms (sum error, sum iterations, #failed), reduced by
        # RCCL called from the C ABI (mmx_comm_all_reduce_norms); gloo only in the one-GPU plumbing test
        capi.residual_norms(outputs, norms)
        if comm is not None:
            comm.all_reduce_norms(norms)
        else:
            D.reduce_norms(dist, norms)

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    elapsed_rank = elapsed
    elapsed = D.reduce_max(dist, elapsed, dev)
    db.last_status = outputs["status"]
    db.last_outputs = outputs
    db.pb_last_iterations = outputs["iterations"]
    db.last_elapsed_rank = elapsed_rank
    return elapsed, theta, [float(x) for x in norms.tolist()]


DUMP_BYTES = 63 * 10**6  # --dump-outputs: the per-instance rows stay below this (64 MB in all with the headers and the norms)


def dump_outputs(path, db: DeviceBatch, theta, norms):
    """What the last timed step returned to its caller, as path/<name>.npy in float32 / float64: theta, error, iterations,
    status (one row per instance) and the reduced norms.  Above DUMP_BYTES the rows are a fixed, seeded sample of the
    instances, whose indices go to path/instances.npy."""
    out = db.last_outputs
    rows = {
        "theta": theta.detach().cpu().numpy(),
        "error": out["error"].cpu().numpy().astype(np.float64),
        "iterations": out["iterations"].cpu().numpy().astype(np.float64),
        "status": out["status"].cpu().numpy().astype(np.float64),
    }
    per_instance = sum(a[0].nbytes for a in rows.values())
    if per_instance * db.B > DUMP_BYTES:
        n = DUMP_BYTES // (per_instance + 8)
        idx = np.sort(np.random.default_rng(12345).choice(db.B, size=n, replace=False))
        rows = {k: a[idx] for k, a in rows.items()}
        rows["instances"] = idx.astype(np.float64)
    rows["norms"] = np.asarray(norms, np.float64)
    os.makedirs(path, exist_ok=True)
    for name, a in rows.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def solved_parameters(pb) -> int:
    """Size of the dense system the solver factors (enabled parameters whose column is not structurally zero)."""
    import ctypes as C

    from momentum_amd import capi

    buf = np.zeros(pb.P, np.int32)
    n = C.c_int32(0)
    capi._check(capi.lib().mmx_debug_fused_normal_equations(pb._h, None, None, None, capi.as_ptr(buf, C.c_int32), C.byref(n), None))
    return int(n.value)


def factor_structure(pb):
    """Route of the last solve and, on the wide route, the tile structure its factor ran with (mmx_problem_tile_structure)."""
    route = pb.last_route()
    out = {"route": route, "solved_parameters": solved_parameters(pb)}
    if route == "wide":
        ts = pb.tile_structure()
        out["factor_tiles"] = f"{ts['tiles']} of {ts['dense_tiles']} 16x16 tiles structurally non-zero (columns in elimination order)"
        out["factor_tile_products"] = f"{ts['products']} of {ts['dense_products']}"
    return out


def fused_pmc():
    """PMC figures of the headline kernel from the committed profile (profiles/pmc_fused.json), or None."""
    path = os.path.join(ROOT, "profiles", "pmc_fused.json")
    if not os.path.exists(path):
        return None
    try:
        return json.load(open(path))
    except Exception:
        return None


def compact_check(chk):
    """What the bench line keeps of a parity check (the rest goes to the side file)."""
    if not chk:
        return {}
    out = {"within_bound": chk["within_bound"], "max_rel": chk["max_rel_theta_vs_oracle_f64"], "median_rel": chk["median_rel_theta_vs_oracle_f64"], "pass": chk["pass"]}
    for k in ("pass_relaxed", "lm_branch_flips", "same_decisions", "num_above_bound_with_same_decisions", "max_rel_same_decisions",
              "flips_double_rho_within_1e-2_of_threshold", "flip_max_abs_rho_difference"):  # fmt: skip
        if k in chk:
            out[k] = chk[k]
    return out


PRECISIONS = ["f32", "f64", "auto", "mixed"]  # MMX_PRECISION_*


def run_extra(key, config, B, line_search, steps, cpu_sample, device_index, iterations, check_n, with_cpu, regularization=0.05, dtype="f32", precision=0, driver_defaults=False):
    """One side configuration: (compact entry of the bench line, details for the side file)."""
    from momentum_amd._abi import GnOptions

    rig, parents, _, step_rule, desc = build_rig(config)
    db = DeviceBatch(rig, parents, B, device_index, 424242, tracker=CONFIGS[config][1].endswith("+tracker"))
    if driver_defaults:
        opt = GnOptions.make(step_rule=step_rule, precision=precision, **DRIVER_DEFAULTS)
        iterations = DRIVER_DEFAULTS["max_iterations"]
    else:
        opt = GnOptions.make(min_iterations=iterations, max_iterations=iterations, threshold=1.0, regularization=regularization, step_rule=step_rule,
                             do_line_search=line_search, precision=precision)  # fmt: skip
    elapsed, theta, norms = solve_loop(db, opt, steps, 1, dtype=dtype)
    status = db.last_status
    chk = parity_check(db, theta, opt, check_n, line_search_aware=line_search != 0)
    n_solved = solved_parameters(db.pb)
    dense_flops = dense_equivalent_flops_per_iteration(db.pb.M, n_solved, rig.num_joints) * iterations
    details = {
        "workload": desc,
        "dtype": dtype,
        "regularization": regularization,
        "batch": B,
        "line_search": line_search,
        "precision": PRECISIONS[precision],
        "step_rule": "lm_schedule" if step_rule == 1 else "gn_fixed_lambda",
        "solves_per_s": B * steps / elapsed,
        "ms_per_step": 1e3 * elapsed / steps,
        "steps": steps,
        "failed_instances": norms[2],
        # informational status bits (include/mmx.h): the factor's damping floor engaged / the precision estimate exceeded the
        # bound / MMX_PRECISION_AUTO re-solved the element in double
        "damping_floored_instances": int((status & 4 != 0).sum()) if status is not None else None,
        "precision_suspect_instances": int((status & 8 != 0).sum()) if status is not None else None,
        "escalated_f64_instances": int((status & 16 != 0).sum()) if status is not None else None,
        "mixed_instances": int((status & 32 != 0).sum()) if status is not None else None,
        "check": chk,
        "solver": factor_structure(db.pb) if dtype == "f32" else {"route": "mmx_solve_f64", "solved_parameters": n_solved},
        "dense_equivalent_tflops": B * steps / elapsed * dense_flops / 1e12,
    }
    if step_rule == 1 and dtype == "f32" and chk:
        # the LM schedule's decisions, exactly: (lambda, rho) per iteration from the GPU against the double oracle's
        n = int(chk["instances"])
        g = db.pb.solve(db.theta0.clone(), opt, want_history=True, want_step_history=True)
        from oracle import oracle as orc

        ref = orc.solve_batch(db.rig, db.host_constraints(n), db.theta0[:n].cpu().numpy(), opt, dtype="f64", nthreads=usable_cores(), step_history=True)
        th = g["theta"][:n].cpu().numpy().astype(np.float64)
        rel = np.linalg.norm(th - ref["theta"], axis=1) / np.maximum(np.linalg.norm(ref["theta"], axis=1), 1e-30)
        lm = lm_branch_analysis(g["step_history"][:n].cpu().numpy(), g["error_history"][:n].cpu().numpy(), ref, rel)
        chk.update(lm)  # (`pass` becomes: 1e-5 wherever the decisions are the double run's)
    compact = {
        "solves_per_s": details["solves_per_s"],
        "ms_per_step": details["ms_per_step"],
        "route": details["solver"]["route"],
        **compact_check(chk),
    }
    if precision in (2, 3):
        compact["escalated_f64"], compact["mixed"] = details["escalated_f64_instances"], details["mixed_instances"]
        compact["precision_suspect"] = details["precision_suspect_instances"]  # (mixed: conjugate gradients that met their step limit)
    if dtype == "f32" and precision == 0:
        compact["precision_suspect"] = details["precision_suspect_instances"]
    if driver_defaults:
        # convergence-driven exits: how many iterations the elements took (solver.cpp:96-119), and whether the oracle's double run
        # took the same number on the checked ones
        its = db.pb_last_iterations.cpu().numpy() if getattr(db, "pb_last_iterations", None) is not None else None
        if its is not None:
            vals, cnt = np.unique(its, return_counts=True)
            compact["iterations_mean"] = float(its.mean())
            compact["iterations_histogram"] = [[int(v), int(c)] for v, c in zip(vals, cnt)]
            compact["options"] = "lambda=0.01 min=4 max=50 threshold=10 line_search=2 (solver_options.h:28-37)"
            if chk and "oracle_iterations" in chk:
                compact["iterations_equal_oracle"] = f"{int((its[: len(chk['oracle_iterations'])] == np.asarray(chk['oracle_iterations'])).sum())}/{len(chk['oracle_iterations'])}"
                details["oracle_iterations_histogram"] = [[int(v), int(c)] for v, c in zip(*np.unique(chk["oracle_iterations"], return_counts=True))]
                del chk["oracle_iterations"]
    if config == "cfg5":
        compact["jtj_dense_equivalent_tflops"] = B * steps / elapsed * iterations * float(db.pb.M) * n_solved * n_solved / 1e12
    if with_cpu:
        c, d = cpu_baseline(db, cpu_sample, opt, dtype, dense_flops)
        details["cpu_baseline"] = d
        details["gpu_over_cpu"] = details["solves_per_s"] / c["value"]
        compact["cpu_value"], compact["cpu_cores"], compact["gpu_over_cpu"] = c["value"], c["cores"], details["gpu_over_cpu"]
    del db
    torch.cuda.empty_cache()
    return compact, details


def measure_traffic(config, B):
    """HBM bytes per launch of the J-assembly kernel from the PMC counters, measured now: two separate rocprofv3 --pmc passes
    (FETCH_SIZE, WRITE_SIZE; no trace options beside them) over scripts/pmc_traffic.py, which launches mmx_eval_jacobian
    on this shape a few times; unit and gfx950 correction as MI355X_MICROARCH.md's HBM section prescribes (counters in KiB-
    like 1024-byte units here; FETCH_SIZE under-reports 2x on gfx950): bytes = 1024 x (WRITE_SIZE + 2 FETCH_SIZE).
    None when rocprofv3 is not available or a pass fails."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rp):
        return None
    vals = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
            cmd = [rp, "--pmc", counter, "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.join(ROOT, "scripts", "pmc_traffic.py"), config, str(B)]
            try:
                subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240, check=True)
            except Exception:
                return None
            per = []
            for path in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if "fkJacobianKernel" in row.get("Kernel_Name", "") and row.get("Counter_Name") == counter:
                        per.append(float(row["Counter_Value"]))
            if not per:
                return None
            vals[counter] = float(np.mean(per[1:] if len(per) > 1 else per))  # (the first launch warms the L2s)
    return 1024.0 * (vals["WRITE_SIZE"] + 2.0 * vals["FETCH_SIZE"])


SHORT = {  # compact workload names of the bench line (the full descriptions: CONFIGS / the details file)
    "cfg2": "BASELINE configs[1]: B x 72-joint humanoid, P=128, pos+ori on 16 landmarks (M=192), GN lambda=0.05, 10 it",
    "cfg3": "BASELINE configs[2]: 65536 x 72-joint, LM schedule, 10 it",
    "cfg4": "BASELINE configs[3]: 32768 x 72-joint per GPU (weak scaling), GN lambda=0.05, 10 it",
    "cfg5": "BASELINE configs[4]: 8192 x 300-joint rig, P=300, M=900, GN lambda=0.05, 10 it",
}


def build_stamp():
    """Which pipeline the solve kernels of the loaded library were compiled with (momentum_amd/build_info.json): the headline
    depends on two internal -mllvm switches; a toolchain that rejects them gets the default pipeline, and the line says so."""
    try:
        from momentum_amd import build as mbuild

        info = mbuild.build_info()
        return {"solve_kernel_pipeline": info.get("solve_kernel_pipeline", "unknown"), "flags_rejected_by_compiler": info.get("flags_rejected_by_compiler")}
    except Exception:
        return {"solve_kernel_pipeline": "unknown"}


def round_floats(x, digits=6):
    """Floats of the bench line to `digits` significant digits (a compact line; nothing is compared at more)."""
    if isinstance(x, float):
        return float(f"{x:.{digits}g}") if np.isfinite(x) else None
    if isinstance(x, dict):
        return {k: round_floats(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [round_floats(v, digits) for v in x]
    return x


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="instances per GPU (default: the config's)")
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=8192)
    ap.add_argument("--check-instances", type=int, default=1024, help="distinct instances of the timed batch re-solved by the oracle (0 = skip)")
    ap.add_argument("--no-extra-configs", action="store_true", help="skip the other BASELINE configurations (N = 1 default run reports them)")
    ap.add_argument("--jac-launches", type=int, default=20)
    ap.add_argument("--measure-traffic", action="store_true", help="measure roofline.traffic in this run (rocprofv3 --pmc over a child process; adds about a minute).  ON by default for the default single-GPU --full run when rocprofv3 is on the path")
    ap.add_argument("--no-measure-traffic", action="store_true", help="never run the rocprofv3 passes: roofline.traffic then comes from the committed pass (profiles/pmc_jacobian.json) and the line says so")
    ap.add_argument("--line-search", type=int, default=0, choices=[0, 1, 2], help="MMX_LINE_SEARCH_*: 0 none (the BASELINE metric), 1 GaussNewtonSolverT's rule, 2 the rule of the batched driver's solvers (SubsetGN / GN-QR)")
    ap.add_argument("--lambda", dest="regularization", type=float, default=0.05, help="GaussNewtonSolverOptions::regularization (the BASELINE metric: 0.05)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"], help="f64: mmx_solve_f64 (SolverT<double>; built for exactness, see DESIGN.md)")
    ap.add_argument("--precision", default="f32", choices=PRECISIONS, help="mmx_gn_options::precision of mmx_solve (mixed: double theta / FK / residuals / g around the single-precision factor; auto: the elements the single-precision solve marks are solved again by the mixed instantiation, what that cannot converge by the double one)")
    ap.add_argument("--driver-defaults", action="store_true", help="the batched driver's real defaults instead of ten fixed iterations (lambda 0.01, 4..50 iterations, threshold 10, line search 2)")
    ap.add_argument("--details", default="", help="where the details of the run go (default gpurun_out/bench_details.json)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step returned (theta, error, iterations, status, the reduced norms) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true", help="everything besides the headline: the J-assembly roofline, the parity check against the CPU oracle, the CPU baseline, the other BASELINE configurations and the details file")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (nccl = RCCL; gloo only for the plumbing test)")
    args = ap.parse_args()

    from momentum_amd import distributed as D

    rank, world, local_rank = D.env_rank()
    if args.gpus != world:
        raise SystemExit(
            f"--gpus {args.gpus} but WORLD_SIZE is {world}: launch N > 1 with torch.distributed.run, one rank per GPU "
            "(python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...)"
        )
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the MI355X path has no CPU fallback")
    # one rank per GPU; --backend gloo with fewer GPUs than ranks is only for the plumbing test
    # (tests/test_bench_two_ranks.py), where the ranks share a device
    local_rank = local_rank % torch.cuda.device_count() if args.backend == "gloo" else local_rank
    torch.cuda.set_device(local_rank)
    dist = D.init(args.backend)  # RCCL behind the "nccl" backend on ROCm; None when world == 1
    comm = None
    if dist is not None and args.backend == "nccl":
        # the data path's exchange goes through the library's own RCCL communicator; torch.distributed only
        # carries the 128-byte id to the other ranks and the barrier of the timing contract
        from momentum_amd import capi

        idt = torch.zeros(capi.COMM_ID_BYTES, dtype=torch.uint8, device=f"cuda:{local_rank}")
        if rank == 0:
            idt.copy_(torch.frombuffer(bytearray(capi.Comm.unique_id()), dtype=torch.uint8))
        dist.broadcast(idt, 0)
        comm = capi.Comm(bytes(idt.cpu().numpy().tobytes()), world, rank, local_rank)
        if comm.world_size != world:  # (what RCCL itself counts: ncclCommCount)
            raise SystemExit(f"RCCL sees {comm.world_size} ranks, --gpus says {world}")

    from momentum_amd._abi import GnOptions

    rig, parents, defB, step_rule, desc = build_rig(args.config)
    B = args.batch if args.batch > 0 else defB
    seed = 12345 + 1000003 * rank  # every rank solves different instances (its shard of the batch)
    db = DeviceBatch(rig, parents, B, local_rank, seed, tracker=CONFIGS[args.config][1].endswith("+tracker"))
    pb, theta_star = db.pb, db.theta_star
    opt = GnOptions.make(min_iterations=args.iterations, max_iterations=args.iterations, threshold=1.0, regularization=args.regularization, step_rule=step_rule,
                         do_line_search=args.line_search, precision=PRECISIONS.index(args.precision))  # fmt: skip
    if args.driver_defaults:
        opt = GnOptions.make(step_rule=step_rule, precision=PRECISIONS.index(args.precision), **DRIVER_DEFAULTS)
    dev = pb.device
    elapsed, theta_final, (total_err, total_it, failed) = solve_loop(db, opt, args.steps, args.warmup, dist, comm, args.dtype)
    # per-rank rates (each rank's own clock around the same K steps) next to the aggregate, which uses the slowest rank's time
    rank_rate_min, rank_rate_max = D.reduce_min_max(dist, float(B) * args.steps / db.last_elapsed_rank, pb.device)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, db, theta_final, (total_err, total_it, failed))

    M, P = pb.M, pb.P
    if args.full:
        # ---- roofline of the J-assembly kernel (mmx_eval_jacobian): HIP events on the launch stream
        Kp_, Ko_ = len(parents[0]), len(parents[1])
        jac = torch.empty((B, P, M), dtype=torch.float32, device=dev)
        res = torch.empty((B, M), dtype=torch.float32, device=dev)
        err = torch.empty((B,), dtype=torch.float64, device=dev)
        for _ in range(3):
            pb.eval_jacobian(theta_star, jac, res, err)
        torch.cuda.synchronize()
        # HIP events attached to the kernel's own dispatch packet on the launch stream
        # (mmx_eval_jacobian_timed -> hipExtLaunchKernelGGL): the kernel's duration as a rocprofv3 kernel
        # trace reports it, without launch latency or the gap between back-to-back dispatches
        jac_ms = float(np.mean([pb.eval_jacobian_kernel_ms(theta_star, jac, res, err) for _ in range(args.jac_launches)]))
        # the same launches bracketed by ordinary recorded events (includes the dispatch latency): reported as context
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.jac_launches)]
        for a, b in evs:
            a.record()
            pb.eval_jacobian(theta_star, jac, res, err)
            b.record()
        torch.cuda.synchronize()
        jac_ms_recorded = float(np.mean([a.elapsed_time(b) for a, b in evs]))
        bytes_per_launch = B * algorithmic_bytes_per_instance(M, P, Kp_, Ko_)
        achieved = bytes_per_launch / (jac_ms * 1e-3) / 1e9
        # HBM traffic of the kernel: measured in THIS run when --measure-traffic is given (two rocprofv3 --pmc passes over a child
        # process that launches the same kernel on the same shape, scripts/pmc_traffic.py); otherwise the committed pass of the
        # same shape (profiles/pmc_jacobian.json), and the line says which
        traffic, traffic_source = None, None
        default_shape = world == 1 and args.config == "cfg2" and args.batch == 0
        want_traffic = (args.measure_traffic or default_shape) and not args.no_measure_traffic
        if want_traffic and rank == 0 and world == 1:
            traffic = measure_traffic(args.config, B)
            traffic_source = "rocprofv3 --pmc in this run" if traffic is not None else None
        pmc_path = os.path.join(ROOT, "profiles", "pmc_jacobian.json")
        if traffic is None and os.path.exists(pmc_path):
            try:
                pm = json.load(open(pmc_path))
                if pm.get("batch") == B and pm.get("config") == args.config:
                    traffic = pm.get("hbm_bytes_per_launch")
                    traffic_source = "profiles/pmc_jacobian.json (committed rocprofv3 --pmc pass of this shape)"
            except Exception:
                traffic = None
        del jac
        # context for the roofline: (i) the same kernel at the weak-scaling shard size of BASELINE
        # configs[3] (32768 instances per GPU), where launch ramp-up and the FK prologue are amortised,
        # (ii) what a plain write-only fill of the same byte count reaches on this box
        extra = {}
        if rank == 0 and world == 1:
            def timed(fn, n):
                for _ in range(2):
                    fn()
                pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
                for a, b in pairs:
                    a.record()
                    fn()
                    b.record()
                torch.cuda.synchronize()
                return float(np.mean([a.elapsed_time(b) for a, b in pairs]))

            fill = torch.empty(bytes_per_launch // 4, dtype=torch.float32, device=dev)
            fill_ms = timed(lambda: fill.zero_(), 5)
            extra["fill_same_bytes_gbs"] = bytes_per_launch / (fill_ms * 1e-3) / 1e9
            # the same stores (layout, workgroup shape, width) without any kinematics: what the write
            # pattern of a column-major J per instance allows on this box
            if M == 3 * (Kp_ + 3 * Ko_):  # (the probe replays the stores of position / orientation rows only)
                for _ in range(2):
                    pb.store_pattern_kernel_ms(fill)
                sp_ms = float(np.mean([pb.store_pattern_kernel_ms(fill) for _ in range(5)]))
                extra["store_pattern_gbs"] = B * 4 * M * P / (sp_ms * 1e-3) / 1e9
            del fill
            if args.config == "cfg2":
                for BL in (32768, 65536):  # the weak-scaling shard of BASELINE configs[3] and north_star's target size
                    if B >= BL:
                        continue
                    dbL = DeviceBatch(rig, parents, BL, local_rank, seed + 1)
                    jacL = torch.empty((BL, P, M), dtype=torch.float32, device=dev)
                    resL = torch.empty((BL, M), dtype=torch.float32, device=dev)
                    errL = torch.empty((BL,), dtype=torch.float64, device=dev)
                    for _ in range(2):
                        dbL.pb.eval_jacobian(dbL.theta_star, jacL, resL, errL)
                    msL = float(np.mean([dbL.pb.eval_jacobian_kernel_ms(dbL.theta_star, jacL, resL, errL) for _ in range(5)]))
                    gbsL = BL * algorithmic_bytes_per_instance(M, P, Kp_, Ko_) / (msL * 1e-3) / 1e9
                    extra[f"at_batch_{BL}"] = {"achieved": gbsL, "frac": gbsL / HBM_PEAK_GBS, "ms_per_launch": msL}
                    del jacL, resL, errL, dbL
                    torch.cuda.empty_cache()
            if args.config == "cfg2" and not args.no_extra_configs:
                # ... and on SURVEY 8(d)'s stress variant (P = 219, both constraints on all 72 joints: M = 864, 766 380 B per instance);
                # (not in the profiling passes, --no-extra-configs: the same kernel name at the same grid size would blur their averages)
                rigA, parA, _, _, _ = build_rig("cfg2_all")
                dbA = DeviceBatch(rigA, parA, 4096, local_rank, seed + 2)
                MA, PA = dbA.pb.M, dbA.pb.P
                jacA = torch.empty((4096, PA, MA), dtype=torch.float32, device=dev)
                resA = torch.empty((4096, MA), dtype=torch.float32, device=dev)
                errA = torch.empty((4096,), dtype=torch.float64, device=dev)
                for _ in range(2):
                    dbA.pb.eval_jacobian(dbA.theta_star, jacA, resA, errA)
                msA = float(np.mean([dbA.pb.eval_jacobian_kernel_ms(dbA.theta_star, jacA, resA, errA) for _ in range(5)]))
                bpiA = algorithmic_bytes_per_instance(MA, PA, len(parA[0]), len(parA[1]))
                gbsA = 4096 * bpiA / (msA * 1e-3) / 1e9
                extra["cfg2_all_at_batch_4096"] = {"achieved": gbsA, "frac": gbsA / HBM_PEAK_GBS, "ms_per_launch": msA, "bytes_per_instance": bpiA}
                del jacA, resA, errA, dbA
                torch.cuda.empty_cache()

    if rank == 0:
        solves = float(B) * world * args.steps
        n_solved = solved_parameters(pb)
        dense_flops = dense_equivalent_flops_per_iteration(M, n_solved, rig.num_joints) * args.iterations
        per_gpu_solves_per_s = float(B) * args.steps / elapsed
        status = db.last_status
        # ONE compact JSON line (the driver keeps its tail): per configuration the rate, the parity figures and the CPU figure;
        # everything else -- above-bound arrays, branch-flip lists, oracle build sweeps, notes -- goes to `details`, written to
        # gpurun_out/bench_details.json (or --details) and summarised on stderr.
        details = {"workload": desc, "switches": {k: v for k, v in sorted(os.environ.items()) if k.startswith("MMX_")}, "configs": {}}
        line = {
            "metric": f"character IK solves/sec ({rig.num_joints}-joint, {args.iterations} GN iters)",
            "value": solves / elapsed,
            "unit": "solves/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "workload": SHORT.get(args.config, args.config),
                "batch_per_gpu": B,
                "global_batch": B * world,
                "joints": rig.num_joints,
                "params": P,
                "rows": M,
                "solved_parameters": n_solved,
                "route": factor_structure(pb)["route"],
                "gn_iterations": args.iterations,
                "line_search": args.line_search,
                "regularization": args.regularization,
                "precision": args.precision,
                "exchange": {
                    "what": "one all-reduce of 3 doubles per solve (sum error, sum iterations, failed)",
                    "backend": "rccl" if comm is not None else ("none" if world == 1 else "gloo"),
                    "ranks_seen_by_rccl": comm.world_size if comm is not None else None,
                    "per_rank_solves_per_s": [rank_rate_min, rank_rate_max],
                },
            },
            "check": {"sum_final_error": total_err, "sum_iterations": total_it, "failed_instances": failed,
                      "damping_floored": int((status & 4 != 0).sum()), "precision_suspect": int((status & 8 != 0).sum()),
                      "escalated_f64": int((status & 16 != 0).sum()), "mixed": int((status & 32 != 0).sum())},
            "build": build_stamp(),
            "roofline_fused": {
                "kernel": "fusedSolveKernel (mmx_solve; latency-bound, no J formed)",
                "dense_equivalent_flops_per_solve": dense_flops,
                "achieved": per_gpu_solves_per_s * dense_flops / 1e12,
                "peak": FP32_PEAK_TFLOPS,
                "unit": "TFLOP/s (dense-equivalent)",
                "frac": per_gpu_solves_per_s * dense_flops / 1e12 / FP32_PEAK_TFLOPS,
            },
        }
    if rank == 0 and not args.full:
        print(json.dumps(round_floats(line), separators=(",", ":")), flush=True)
    if rank == 0 and args.full:
        line["roofline"] = {
            "kernel": "fkJacobianKernel<true> (mmx_eval_jacobian)",
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_source": traffic_source,
            "bytes_per_launch": bytes_per_launch,
            "ms_per_launch": jac_ms,
            "batch": B,
            **extra,
        }
        details["roofline_fused_pmc"] = fused_pmc()
        details["roofline_timing"] = {"ms_per_launch_recorded_events": jac_ms_recorded, "how": "HIP events attached to the kernel's dispatch packet on the launch stream (hipExtLaunchKernelGGL)"}
        if args.check_instances > 0:
            chk = parity_check(db, theta_final, opt, args.check_instances)
            details["check"] = chk
            line["check"].update(compact_check(chk))
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"], details["cpu_baseline"] = cpu_baseline(db, args.cpu_sample, opt, args.dtype, dense_flops)
        default_run = world == 1 and args.config == "cfg2" and args.batch == 0 and args.line_search == 0 and args.dtype == "f32" and args.precision == "f32" and not args.driver_defaults
        if default_run and not args.no_extra_configs:
            del db, pb
            torch.cuda.empty_cache()
            line["configs"] = {}
            for key, cfg, eb, ls, steps, sample, lam, *rest in EXTRA_RUNS:
                try:
                    line["configs"][key], details["configs"][key] = run_extra(key, cfg, eb, ls, steps, sample, local_rank, args.iterations, args.check_instances, not args.no_cpu_baseline, lam, *rest)
                except Exception as ex:  # a failing side configuration must not lose the headline line
                    line["configs"][key] = {"error": f"{type(ex).__name__}: {ex}"[:200]}
        line = round_floats(line)
        try:
            path = args.details or os.path.join(ROOT, "gpurun_out", "bench_details.json")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                json.dump(dict(details, line=line), f, indent=1)
            print(f"[bench] details: {path}", file=sys.stderr)
        except OSError as ex:
            print(f"[bench] details not written: {ex}", file=sys.stderr)
        for key, c in line.get("configs", {}).items():
            print(f"[bench] {key:52s} {c.get('solves_per_s', 0):.4g} solves/s  within {c.get('within_bound')}  max_rel {c.get('max_rel')}  pass {c.get('pass')}", file=sys.stderr)
        print(json.dumps(line, separators=(",", ":")), flush=True)
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
