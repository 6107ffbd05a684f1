"""Rate of a keypoint-shaped problem next to cfg2's: the cfg2 rig (72-joint humanoid, P = 128) with its 16 landmark joints
seen as 2D keypoints through two cameras (32 projection constraints, MMX_JC_PROJECTION) instead of position + orientation
constraints, B = 4096, the one-launch route, Gauss-Newton lambda = 0.05, 10 iterations; cfg2 itself timed the same way.
Prints one JSON line (solves per second = B x steps / elapsed).

    python scripts/keypoint_rate.py [--steps 20] [--warmup 3] [--batch 4096]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(torch, pb, theta0, opt, steps, warmup):
    for _ in range(warmup):
        pb.solve(theta0.clone(), opt)
    torch.cuda.synchronize()
    thetas = [theta0.clone() for _ in range(steps)]
    t0 = time.perf_counter()
    for th in thetas:
        pb.solve(th, opt)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, pb.last_route()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    import torch

    import bench
    from momentum_amd import capi
    from momentum_amd._abi import GnOptions
    from tests import projection_reference as pr

    B = a.batch
    opt = GnOptions.make(min_iterations=10, max_iterations=10, threshold=1.0, regularization=0.05)
    rig, parents, _, _, _ = bench.build_rig("cfg2")
    db = bench.DeviceBatch(rig, parents, B, 0, 12345)
    db.pb.set_route("fused")
    dt2, route2 = timed(torch, db.pb, db.theta0, opt, a.steps, a.warmup)
    lm = parents[0]
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 12345, [], lm, n_cams=2)
    pb = capi.Problem(capi.RigHandle(rig, 0), B, [], [])
    dev = pb.device
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    blk = blocks[0]
    gb = [type(blk)(blk.type, blk.parent, t(blk.weight), t(blk.global_), t(blk.local_point), projection=t(blk.projection), near_clip=blk.near_clip)]
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    pb.set_constraints(z(B, 0, 3), z(B, 0, 3), z(B, 0), z(B, 0, 4), z(B, 0, 4), z(B, 0), joint_blocks=gb)
    pb.set_route("fused")
    dtk, routek = timed(torch, pb, t(th0), opt, a.steps, a.warmup)
    out = pb.solve(t(th0), opt)
    print(json.dumps({
        "metric": "solves_per_s", "batch": B, "steps": a.steps, "iterations": 10,
        "cfg2": {"solves_per_s": B * a.steps / dt2, "ms_per_step": 1e3 * dt2 / a.steps, "route": route2, "rows": int(db.pb.M)},
        "keypoints_2cams": {"solves_per_s": B * a.steps / dtk, "ms_per_step": 1e3 * dtk / a.steps, "route": routek, "rows": int(pb.M),
                            "failed": int((out["status"] & 3 != 0).sum().item())},
    }))  # fmt: skip


if __name__ == "__main__":
    main()
