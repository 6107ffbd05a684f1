"""Rate of a problem with joint-to-joint distance constraints next to cfg2's, and of the keypoint problem of
scripts/keypoint_rate.py (the existing block types run through the same gather as the pair rows): the cfg2 rig (72-joint
humanoid, P = 128), B = 4096, the one-launch route, Gauss-Newton lambda = 0.05, 10 iterations.

  pairs      cfg2's 16 position constraints plus its 16 landmark joints as 8 pair-distance constraints (spine4 - head and the
             seven left / right pairs: knees, ankles, toes, elbows, wrists, index and thumb tips; MMX_JC_JOINT_TO_JOINT_DISTANCE),
             targets at the ground-truth pose
  cfg2       cfg2 itself (16 position + 16 orientation constraints), timed the same way
  keypoints  the 16 landmarks as 2D keypoints through two cameras (32 MMX_JC_PROJECTION constraints)

Prints one JSON line (solves per second = B x steps / elapsed).  --skip-pairs times cfg2 and the keypoints only: that part
also runs on a library from before the pair type (MMX_LIB=<path>), which is how the figures of two builds are compared.

    python scripts/joint_pair_rate.py [--steps 20] [--warmup 3] [--batch 4096] [--skip-pairs]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--skip-pairs", action="store_true")
    a = ap.parse_args()
    import torch

    import bench
    from keypoint_rate import timed
    from momentum_amd import _abi, capi
    from momentum_amd._abi import GnOptions, JointBlock
    from tests import projection_reference as pr

    B = a.batch
    opt = GnOptions.make(min_iterations=10, max_iterations=10, threshold=1.0, regularization=0.05)
    rig, parents, _, _, _ = bench.build_rig("cfg2")
    lm = parents[0]
    rate = lambda dt, route, pb, **kw: {"solves_per_s": B * a.steps / dt, "ms_per_step": 1e3 * dt / a.steps, "route": route, "rows": int(pb.M), **kw}
    failed = lambda pb, th: int((pb.solve(th.clone(), opt)["status"] & 3 != 0).sum().item())
    result = {"metric": "solves_per_s", "batch": B, "steps": a.steps, "iterations": 10, "library": os.environ.get("MMX_LIB", "")}

    db = bench.DeviceBatch(rig, parents, B, 0, 12345)
    db.pb.set_route("fused")
    dt, route = timed(torch, db.pb, db.theta0, opt, a.steps, a.warmup)
    result["cfg2"] = rate(dt, route, db.pb)

    if not a.skip_pairs:
        dp = bench.DeviceBatch(rig, (lm, []), B, 0, 12345)  # cfg2's position constraints, targets at theta*
        pb, dev = dp.pb, dp.pb.device
        ja, jb = np.asarray(lm[0::2], np.int32), np.asarray(lm[1::2], np.int32)
        st = pb.skeleton_state(dp.theta_star)
        idx = lambda j: torch.as_tensor(j.astype(np.int64), device=dev)
        dist = (st[:, idx(ja), 0:3] - st[:, idx(jb), 0:3]).norm(dim=-1).contiguous()
        z3 = torch.zeros((B, len(ja), 3), device=dev)
        blk = JointBlock(_abi.MMX_JC_JOINT_TO_JOINT_DISTANCE, ja, torch.ones((B, len(ja)), device=dev), None, local_point=z3, local_dir=z3.clone(),
                         plane_d=dist, parent_b=jb)  # fmt: skip
        pb.set_constraints(dp.pos_offset, dp.pos_target, dp.pos_weight, dp.ori_offset, dp.ori_target, dp.ori_weight, joint_blocks=[blk])
        pb.set_route("fused")
        dt, route = timed(torch, pb, dp.theta0, opt, a.steps, a.warmup)
        result["pairs_8_plus_positions"] = rate(dt, route, pb, failed=failed(pb, dp.theta0))

    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 12345, [], lm, n_cams=2)
    pb = capi.Problem(capi.RigHandle(rig, 0), B, [], [])
    dev = pb.device
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    blk = blocks[0]
    gb = [JointBlock(blk.type, blk.parent, t(blk.weight), t(blk.global_), t(blk.local_point), projection=t(blk.projection), near_clip=blk.near_clip)]
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    pb.set_constraints(z(B, 0, 3), z(B, 0, 3), z(B, 0), z(B, 0, 4), z(B, 0, 4), z(B, 0), joint_blocks=gb)
    pb.set_route("fused")
    dt, route = timed(torch, pb, t(th0), opt, a.steps, a.warmup)
    result["keypoints_2cams"] = rate(dt, route, pb, failed=failed(pb, t(th0)))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
