"""Gradient + error of a batch: one Problem.eval_gradient call (mmx_eval_gradient: through the tree, no Jacobian) against what a
caller writes without it -- Problem.eval_jacobian into preallocated buffers, then 2 J^T r contracted on the device with
torch.bmm --, same process, same build, same seeded device payload.

Shapes: BASELINE configs[1] (72-joint humanoid, P = 128, both constraints on the 16 landmarks, M = 192) at B = 4096 and 65 536,
its all-joints stress variant (P = 219, M = 864) at 4096, and the 3-joint character at 65 536.  The script checks that the two
ways agree to single-precision rounding.  Per shape the two alternate: two warm-up calls each, then five rounds each, every round
timed with device events around at least 0.3 s of calls.  Written per shape and way: median / min / max evaluations/s (an
evaluation = one instance's error and gradient), the ratio of the medians, the round-to-round spread of the Jacobian way.
    python scripts/gradient_rate.py [--out profiles/gradient_rate.json] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from momentum_amd import capi, humanoid72_landmark_joints, make_humanoid72, make_test_character  # noqa: E402
from tests.helpers import make_problem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradient_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small batches (rehearsal); nothing is written")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 256  # distinct seeded instances, tiled over the batch
UNIT = 0.01  # bench.py's unit


def shapes():
    p128 = make_humanoid72(seed=12345, variant="p128", unit=UNIT)
    lm = humanoid72_landmark_joints(p128)
    p219 = make_humanoid72(seed=12345, variant="p219", unit=UNIT)
    allj = np.arange(p219.num_joints, dtype=np.int32)
    char3 = make_test_character(3)
    j3 = np.arange(3, dtype=np.int32)
    return [
        ("configs[1] 72-joint humanoid P=128 M=192", p128, lm, lm, 4096),
        ("configs[1] 72-joint humanoid P=128 M=192", p128, lm, lm, 65536),
        ("configs[1] stress variant P=219 M=864 (all joints)", p219, allj, allj, 4096),
        ("3-joint character P=10 M=36", char3, j3, j3, 65536),
    ]


def timed(run, count, seconds):
    """evaluations/s over a window of at least `seconds` (device events around the whole window)"""
    n, done, ms = 1, 0, 0.0
    while ms < 1e3 * seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            run()
        e1.record()
        e1.synchronize()
        ms, done = e0.elapsed_time(e1), n
        n *= 2
    return count * done / (1e-3 * ms)


assert torch.cuda.is_available(), "gradient_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "unit": "evaluations/s (one instance's error and gradient)", "shapes": {}}
for name, rig, pp, op, B in shapes():
    if args.quick:
        B = min(B, 512)
    cons, th0, _ = make_problem(rig, pp, op, D, seed=12345, perturb=0.3, random_offsets=True, weights="random", theta0_scale=0.2, offset_scale=UNIT if rig.num_joints > 3 else 1.0)
    P = rig.num_params
    idx = torch.arange(B, device=dev) % D
    payload = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)[idx].contiguous()
               for a in (cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_offset, cons.ori_target, cons.ori_weight)]  # fmt: skip
    theta = torch.from_numpy(th0).to(dev)[idx].contiguous()
    pb = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
    pb.set_constraints(*payload)
    M = pb.M
    jac = torch.empty((B, P, M), dtype=torch.float32, device=dev)
    res = torch.empty((B, M), dtype=torch.float32, device=dev)
    errj = torch.empty((B,), dtype=torch.float64, device=dev)
    gj = torch.empty((B, P, 1), dtype=torch.float32, device=dev)
    grad = torch.empty((B, P), dtype=torch.float32, device=dev)
    err = torch.empty((B,), dtype=torch.float64, device=dev)

    def run_jacobian():
        pb.eval_jacobian(theta, jac=jac, res=res, err=errj)
        torch.bmm(jac, res.unsqueeze(2), out=gj)
        gj.mul_(2.0)

    def run_gradient():
        pb.eval_gradient(theta, grad=grad, err=err)

    ways = {"eval_gradient": run_gradient, "eval_jacobian_bmm": run_jacobian}
    for run in ways.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    gs = gj[:, :, 0].abs().amax(dim=1).clamp_min(1e-30)
    dg = float(((grad - gj[:, :, 0]).abs().amax(dim=1) / gs).max())
    de = float(((err - errj).abs() / errj).max())
    assert dg <= 1e-5 and de <= 1e-5, (name, B, dg, de)  # single-precision rounding (the tests hold the real bound)
    row = {"batch": B, "P": P, "M": M, "jacobian_bytes_per_instance": 4 * M * P, "max_rel_gradient_difference": dg, "max_rel_error_difference": de}
    rates = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, run in ways.items():
            rates[k].append(timed(run, B, WINDOW))
    for k in rates:
        r = np.array(rates[k])
        row[k] = dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()))
    jr = np.array(rates["eval_jacobian_bmm"])
    row["jacobian_spread"] = float((jr.max() - jr.min()) / np.median(jr))
    row["gradient_over_jacobian"] = row["eval_gradient"]["median"] / row["eval_jacobian_bmm"]["median"]
    result["shapes"][f"{name} @ B={B}"] = row
    print(f"{name} @ B={B}: eval_gradient {row['eval_gradient']['median']:.4g} eval_jacobian+bmm {row['eval_jacobian_bmm']['median']:.4g} evaluations/s"
          f"  x{row['gradient_over_jacobian']:.2f}  (Jacobian-way spread {100 * row['jacobian_spread']:.1f} %; outputs differ by {dg:.1e} / {de:.1e})", flush=True)  # fmt: skip
    pb.close()
    del payload, jac, res, gj, grad
    torch.cuda.empty_cache()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
