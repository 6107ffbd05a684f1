"""A/B of mmx_tuning::joint_pruning in ONE process on one GPU: bench.py's device batches of cfg2 @ 4096, cfg3 @ 65536 (LM
schedule) and cfg2 @ 4096 with the directional line search, the switch alternating off / on.

Per shape: warm-up, then the SAME setting (on) timed twice -- the spread of this box --, then `--rounds` rounds of off / on,
every window `--steps` solves with a device synchronise inside the clock.  The change counts as a gain when the headline's
median improvement exceeds twice the same-setting spread.  The two settings' results are compared bit for bit as well.
    python scripts/ab_joint_pruning.py [--steps 30] [--rounds 3] [--out profiles/r07_joint_pruning_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from momentum_amd._abi import GnOptions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_joint_pruning_ab.txt"))
args = ap.parse_args()
assert args.steps >= 30 and args.rounds >= 3

SHAPES = [("cfg2@4096", "cfg2", 4096, 0, 0), ("cfg3@65536 (LM schedule)", "cfg3", 65536, 1, 0), ("cfg2@4096 line search 2", "cfg2", 4096, 0, 2)]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(db, opt, pruning, steps):
    """solves/s of `steps` solves with the switch set; returns (rate, theta, error, iterations, status of the last one)"""
    pb = db.pb
    pb.set_joint_pruning(pruning)
    theta = db.theta0.clone()
    out = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        theta.copy_(db.theta0)
        out = pb.solve(theta, opt)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return db.B * steps / dt, out


say(f"joint pruning A/B, one process, {args.steps} solves per window, {args.rounds} rounds of off / on; device: {torch.cuda.get_device_name(0)}")
for name, cfg, B, rule, ls in SHAPES:
    rig, parents, _, _, _ = bench.build_rig(cfg)
    db = bench.DeviceBatch(rig, parents, B, 0, 12345)
    opt = GnOptions.make(min_iterations=10, max_iterations=10, threshold=1.0, regularization=0.05, step_rule=rule, do_line_search=ls)
    db.pb.set_joint_pruning(True)
    live = db.pb.num_solve_joints()
    for pr in (False, True):
        window(db, opt, pr, args.warmup)
    same = [window(db, opt, True, args.steps)[0] for _ in range(2)]
    spread = abs(same[0] - same[1]) / min(same)
    off, on = [], []
    res = {}
    for _ in range(args.rounds):
        for pr, acc in ((False, off), (True, on)):
            rate, out = window(db, opt, pr, args.steps)
            acc.append(rate)
            res[pr] = {k: out[k].clone() for k in ("theta", "error", "iterations", "status")}
    equal = all(torch.equal(res[False][k], res[True][k]) for k in res[True])
    moff, mon = statistics.median(off), statistics.median(on)
    gain = mon / moff - 1.0
    say(f"{name}: joints {rig.num_joints} -> {live} live, route {db.pb.last_route()}")
    say(f"  same setting twice (on): {same[0]:.4e} {same[1]:.4e} solves/s, spread {100 * spread:.2f} %")
    say("  off: " + " ".join(f"{r:.4e}" for r in off) + f"  median {moff:.4e}")
    say("  on:  " + " ".join(f"{r:.4e}" for r in on) + f"  median {mon:.4e}")
    say(f"  on / off - 1 = {100 * gain:+.2f} %   (twice the spread: {200 * spread:.2f} %; a gain: {gain > 2 * spread})   results bit-identical: {equal}")
    del db
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
