"""Forward + backward of a scalar loss of the skeleton state: momentum_amd.autograd.skeleton_state (mmx_eval_skeleton_state and
mmx_eval_skeleton_state_backward: one kernel each) against what a caller writes without it -- the pure-torch level-by-level
forward kinematics of tests/skeleton_state_reference.py in float32 on the device, differentiated by torch autograd --, same
process, same seeded parameters, the same loss L = sum(cotangent * state).

Shapes: the 3-joint character, the 24-joint chain, the 72-joint humanoid (P = 128) and the 300-joint rig, at B = 4096 and
65 536.  The script checks that the two gradients agree to single-precision rounding.  Per shape the two alternate: two warm-up
calls each, then five rounds each, every round timed with device events around at least 0.3 s of calls.  Written per shape and
way: median / min / max evaluations/s (an evaluation = one instance's state and gradient), the ratio of the medians, the
round-to-round spread of either way.
    python scripts/state_backward_rate.py [--out profiles/state_backward_rate.json] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from momentum_amd import autograd as mauto  # noqa: E402
from momentum_amd import capi, make_humanoid72, make_rig300, make_test_character  # noqa: E402
from tests import skeleton_state_reference as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_backward_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small batches (rehearsal); nothing is written")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 256  # distinct seeded instances, tiled over the batch
UNIT = 0.01  # bench.py's unit


def shapes():
    rigs = [
        ("3-joint character P=10", make_test_character(3)),
        ("24-joint chain P=32", make_test_character(24)),
        ("72-joint humanoid P=128", make_humanoid72(seed=12345, variant="p128", unit=UNIT)),
        ("300-joint rig P=300", make_rig300(seed=12345, unit=UNIT)),
    ]
    return [(name, rig, B) for name, rig in rigs for B in (4096, 65536)]


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


assert torch.cuda.is_available(), "state_backward_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "unit": "evaluations/s (one instance's skeleton state and the gradient of a scalar loss of it)", "shapes": {}}
for name, rig, B in shapes():
    if args.quick:
        B = min(B, 512)
    th0, cot0 = ref.random_inputs(rig, D, seed=12345)
    idx = torch.arange(B, device=dev) % D
    theta = torch.from_numpy(th0).to(dev)[idx].contiguous().requires_grad_(True)
    cot = torch.from_numpy(cot0).to(dev)[idx].contiguous()
    pb = capi.Problem(capi.RigHandle(rig, 0), B, [0], [])
    rt = ref.RigTensors(rig, torch.float32, dev)
    grads = {}

    def run_kernels():
        theta.grad = None
        (mauto.skeleton_state(pb, theta) * cot).sum().backward()
        grads["kernels"] = theta.grad

    def run_torch():
        theta.grad = None
        (ref.skeleton_state(rt, theta) * cot).sum().backward()
        grads["torch"] = theta.grad

    ways = {"autograd_skeleton_state": run_kernels, "torch_level_by_level": run_torch}
    for run in ways.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    run_kernels(), run_torch()
    gs = grads["torch"].abs().amax(dim=1).clamp_min(1e-30)
    dg = float(((grads["kernels"] - grads["torch"]).abs().amax(dim=1) / gs).max())
    assert dg <= 2e-5, (name, B, dg)  # single-precision rounding (the tests hold the real bound)
    row = {"batch": B, "J": rig.num_joints, "P": rig.num_params, "levels": len(rt.level_joints), "max_rel_gradient_difference": dg}
    rates = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, run in ways.items():
            rates[k].append(timed(run, B, WINDOW))
    for k in rates:
        r = np.array(rates[k])
        row[k] = dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()), spread=float((r.max() - r.min()) / np.median(r)))
    row["kernels_over_torch"] = row["autograd_skeleton_state"]["median"] / row["torch_level_by_level"]["median"]
    result["shapes"][f"{name} @ B={B}"] = row
    print(f"{name} @ B={B}: autograd.skeleton_state {row['autograd_skeleton_state']['median']:.4g} torch level by level {row['torch_level_by_level']['median']:.4g} evaluations/s"
          f"  x{row['kernels_over_torch']:.2f}  (spreads {100 * row['autograd_skeleton_state']['spread']:.1f} % / {100 * row['torch_level_by_level']['spread']:.1f} %; gradients differ by {dg:.1e})", flush=True)  # fmt: skip
    pb.close()
    del theta, cot, grads
    torch.cuda.empty_cache()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
