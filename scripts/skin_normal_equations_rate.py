"""Gauss-Newton terms of vertex position constraints on every vertex of a skinned mesh: Problem.vertex_normal_equations
(mmx_skin_normal_equations: one kernel, H = J^T J on the matrix cores, J never stored) against what a caller writes without it
-- the float32 torch pipeline of tests/vertex_constraints_reference.py on the device (skeleton_state -> skin_points -> rows), its
dense J [rows x P] from batched-cotangent autograd over the rows (torch.autograd.grad with is_grads_batched, the rows in chunks
so that no temporary of the vmapped backward exceeds 512 MiB and J itself stays within 4 GiB), then torch.bmm for H and g --,
same process, same seeded parameters and targets.

Shapes: the 72-joint humanoid (p128: n = 128) with V = C = 2 000 (K = 4) at 256 and 4096 instances and V = C = 20 000 at 16
instances, the 3-joint character with V = 500 at 4096 instances.  The kernel launches one workgroup per instance: the
16-instance shape occupies 16 of the 256 compute units, and is reported as it comes.  The torch way needs one backward pass
through the whole pipeline per row -- 27 s per call for the 6 000 rows of the V = 2 000 mesh, whether on 4 or on 16 instances --:
it is timed on the first min(B, --torch-batch) instances of the batch, its rate is per instance like the kernel's, and only
--torch-work / V rows of J are built per call (600 at V = 2 000, 60 at V = 20 000), the time scaled by rows / rows built (every row
costs the same backward pass over all V vertices; the shape's entry is marked "extrapolated_from_rows").  The script checks that the two ways agree to
single-precision rounding (where J is built in full; else on the error).  Per shape the two alternate: warm-up calls, then five
rounds each, every round timed with device events around at least 0.3 s of calls (at least one call).  Written per shape and
way: median / min / max instances/s and constraint rows/s, the ratio of the medians, the round-to-round spread of either way.
    python scripts/skin_normal_equations_rate.py [--out profiles/skin_normal_equations_rate.json] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from momentum_amd import capi, make_humanoid72, make_test_character, make_test_skin  # noqa: E402
from tests import skeleton_state_reference as fk  # noqa: E402
from tests import skinning_reference as skr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_normal_equations_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small shapes (rehearsal); nothing is written")
ap.add_argument("--torch-batch", type=int, default=4, help="instances the torch way is timed on")
ap.add_argument("--torch-work", type=float, default=1.2e6, help="rows x V the torch way builds J for per call (more rows: time scaled)")
ap.add_argument("--cpu-rehearsal", action="store_true", help="run the torch way alone on the CPU at a tiny shape and exit")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 64  # distinct seeded instances, tiled over the batch
UNIT = 0.01  # bench.py's unit
TEMP_FLOATS = 2**27  # 512 MiB: the largest temporary of the vmapped backward, [row chunk][instances][V][K][3]


def shapes():
    hum = make_humanoid72(seed=12345, variant="p128", unit=UNIT)
    out = [("72-joint humanoid", hum, 2000, 4, 256), ("72-joint humanoid", hum, 2000, 4, 4096), ("72-joint humanoid", hum, 20000, 4, 16)]
    return out + [("3-joint character", make_test_character(3), 500, 4, 4096)]


def torch_normal_equations(rt, sk, theta, target, row_limit=None):
    """(H [B, P, P], g [B, P], err [B]) of position constraints on every vertex, all weights 1: the dense-J way in float32.
    row_limit: build (and multiply) the first row_limit rows of J only -- for timing; H and g are then partial sums."""
    B, P = theta.shape
    th = theta.detach().clone().requires_grad_(True)
    r = (skr.skin_points(sk, fk.skeleton_state(rt, th)) - target).reshape(B, -1)  # [B, R]
    R = r.shape[1]
    Rb = R if row_limit is None else min(R, row_limit)
    chunk = max(1, min(Rb, TEMP_FLOATS // (B * sk.V * sk.K * 3)))
    J = torch.empty((B, Rb, P), dtype=theta.dtype, device=theta.device)
    for r0 in range(0, Rb, chunk):
        m = min(chunk, Rb - r0)
        cot = torch.zeros((m, B, R), dtype=theta.dtype, device=theta.device)  # cotangent i: row r0 + i of every instance at once
        i = torch.arange(m, device=theta.device)
        cot[i, :, r0 + i] = 1
        (Jc,) = torch.autograd.grad(r, th, grad_outputs=cot, is_grads_batched=True, retain_graph=True)  # [chunk, B, P]
        J[:, r0 : r0 + chunk] = Jc.transpose(0, 1)
    r = r.detach()
    return torch.bmm(J.transpose(1, 2), J), torch.bmm(J.transpose(1, 2), r[:, :Rb, None])[..., 0], (r.double() ** 2).sum(1)


def timed(run, count, seconds):
    """instances/s over a window of at least `seconds` (device events around the whole window)"""
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


def summary(rates, rows):
    r = np.array(rates)
    return dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()), spread=float((r.max() - r.min()) / np.median(r)),
                rows_per_s=float(np.median(r)) * rows)  # fmt: skip


if args.cpu_rehearsal:
    rig = make_test_character(3)
    s = make_test_skin(rig, 7, 2, seed=1)
    rt, sk = fk.RigTensors(rig, torch.float64), skr.SkinTensors(s.joint, s.weight, s.inverse_bind, s.rest, 3, torch.float64)
    th = torch.as_tensor(fk.random_inputs(rig, 2, 3)[0].astype(np.float64))
    tgt = torch.zeros((2, 7, 3), dtype=torch.float64)
    TEMP_FLOATS = 2 * 7 * 2 * 3 * 4  # four rows per chunk
    H, g, e = torch_normal_equations(rt, sk, th, tgt)
    from tests import vertex_constraints_reference as vcr

    want = vcr.normal_equations(rig, (s.joint, s.weight, s.inverse_bind, s.rest), th.numpy(), vcr.Constraints(np.zeros((2, 7, 3), np.float32)))
    print("max differences", np.abs(H.numpy() - want["H"]).max(), np.abs(g.numpy() - want["g"]).max(), np.abs(e.numpy() - want["err"]).max())
    sys.exit(0)

assert torch.cuda.is_available(), "skin_normal_equations_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "torch_batch": args.torch_batch,
          "unit": "instances/s (one instance's H [n x n], g [n] and error of position constraints on all V vertices: 3 V rows); rows_per_s = 3 V x that",
          "shapes": {}}  # fmt: skip
for name, rig, V, K, B in shapes():
    if args.quick:
        B, V = min(B, 32), min(V, 500)
    J, P = rig.num_joints, rig.num_params
    s = make_test_skin(rig, V, K, seed=12345)
    rh = capi.RigHandle(rig, 0)
    skin = capi.Skin(rh, s.joint, s.weight, s.inverse_bind, s.rest)
    pb = capi.Problem(rh, B, [0], [])
    th0, _ = fk.random_inputs(rig, D, seed=12345)
    th1, _ = fk.random_inputs(rig, D, seed=12346)
    idx = torch.arange(B, device=dev) % D
    theta = torch.from_numpy(th0).to(dev)[idx].contiguous()
    # targets: the mesh posed at other parameters (residuals of the size of a pose change)
    pbD = capi.Problem(rh, D, [0], [])
    target = skin.skin_points(pbD.skeleton_state(torch.from_numpy(th1).to(dev)))[idx].contiguous()
    rt = fk.RigTensors(rig, torch.float32, dev)
    sk = skr.SkinTensors(s.joint, s.weight, s.inverse_bind, s.rest, J, torch.float32, dev)
    rows = 3 * V
    Bt = min(B, args.torch_batch)
    Rb = max(1, min(rows, int(args.torch_work // V)))
    got = {}

    def run_kernel():
        got["kernel"] = pb.vertex_normal_equations(skin, theta, target)

    def run_torch():
        got["torch"] = torch_normal_equations(rt, sk, theta[:Bt], target[:Bt], Rb)

    run_kernel(), run_kernel(), run_torch()
    torch.cuda.synchronize()
    dist = []
    for i, (a, b) in enumerate(zip(got["kernel"], got["torch"])):
        a, b = a[:Bt].double().reshape(Bt, -1), b.double().reshape(Bt, -1)
        d = float(((a - b).abs().amax(dim=1) / b.abs().amax(dim=1).clamp_min(1e-30)).max())
        dist.append(d if (Rb == rows or i == 2) else None)  # (a partial J gives partial sums of H and g: only the error compares)
    assert max(d for d in dist if d is not None) <= 1e-3, (name, V, B, dist)  # single-precision rounding of float32 sums over 3 V rows (the tests hold the real bound)
    row = {"batch": B, "torch_batch": Bt, "J": J, "P": P, "V": V, "K": K, "rows": rows, "max_rel_difference_H_g_err": dist}
    if Rb < rows:
        row["extrapolated_from_rows"] = Rb
    got.clear()
    ways = {"vertex_normal_equations": (run_kernel, B), "torch_dense_jacobian": (run_torch, Bt)}
    rates = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, (run, count) in ways.items():
            rates[k].append(timed(run, count, WINDOW))
    rates["torch_dense_jacobian"] = [x * Rb / rows for x in rates["torch_dense_jacobian"]]  # (every row costs the same backward pass)
    for k in rates:
        row[k] = summary(rates[k], rows)
    row["kernel_over_torch"] = row["vertex_normal_equations"]["median"] / row["torch_dense_jacobian"]["median"]
    row["kernel_ms_per_call"] = 1e3 * B / row["vertex_normal_equations"]["median"]
    result["shapes"][f"{name} V={V} @ B={B}"] = row
    print(f"{name} V={V} @ B={B}: kernel {row['vertex_normal_equations']['median']:.4g} instances/s ({row['vertex_normal_equations']['rows_per_s']:.4g} rows/s,"
          f" {row['kernel_ms_per_call']:.3f} ms per call), torch dense J on {Bt} instances {row['torch_dense_jacobian']['median']:.4g} instances/s"
          f"  x{row['kernel_over_torch']:.1f}  (spreads {100 * row['vertex_normal_equations']['spread']:.1f} % / {100 * row['torch_dense_jacobian']['spread']:.1f} %;"
          f" H, g, err differ by {dist})", flush=True)  # fmt: skip
    skin.close(), pb.close(), pbD.close()
    del theta, target, rt, sk
    torch.cuda.empty_cache()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
