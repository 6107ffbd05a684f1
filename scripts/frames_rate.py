"""Frame sequences: one mmx_solve_frames launch against the per-frame loop a caller writes without it, same process, same build,
same seeded device payload.

S sequences of F frames, warm-started along the sequence (the loop of marker_tracker.cpp:905-913).  The two ways:
  frames  one F x S handle, Problem.solve_frames: one launch, a wavefront owns a sequence
  loop    one S-instance handle pinned to the same route ("wave"); per frame set_constraints on that frame's device tensors,
          solve in place, copy the row out
The script asserts that the two give bit-identical parameters.  Per shape the two alternate: two warm-up runs each, then five
rounds each, every round timed with device events around at least 0.3 s of whole-sequence runs.  Written per shape and way:
median / min / max frames/s (a frame = one instance's solve), the ratio of the medians, the loop-vs-loop spread of the rounds.
    python scripts/frames_rate.py [--sequences 64,1024,16384] [--frames 64] [--out profiles/frames_rate.json] [--quick]
"""
import argparse
import json
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from momentum_amd import capi, make_test_character  # noqa: E402
from momentum_amd._abi import GnOptions  # noqa: E402
from tests.helpers import make_problem  # noqa: E402
from tests.test_real_rig import fixture_rig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sequences", default="64,1024,16384")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows (profiler runs); nothing is written")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.05) if args.quick else (5, 0.3)
D = 1024  # distinct seeded instances, tiled over the frames and sequences
F = args.frames

glb = fixture_rig(np.load(os.path.join(ROOT, "tests", "golden", "real_rig_character_with_motion.npz"), allow_pickle=True))
chain = make_test_character(24)
DRIVER = dict(min_iterations=4, max_iterations=50, threshold=10.0, regularization=0.01, do_line_search=2)
SHAPES = [("glb driver defaults", glb, DRIVER), ("chain24 driver defaults", chain, DRIVER)]


def timed(run, frames, seconds):
    """frames/s over a window of at least `seconds` (device events around the whole window)"""
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
    return frames * done / (1e-3 * ms)


result = {"rounds": ROUNDS, "window_seconds": WINDOW, "frames": F, "shapes": {}}
for name, rig, okw in SHAPES:
    jj = np.arange(rig.num_joints, dtype=np.int32)
    cons, th0, _ = make_problem(rig, jj, jj, D, seed=12345, perturb=0.3)
    opt = GnOptions.make(**okw)
    P = rig.num_params
    for S in [int(x) for x in args.sequences.split(",")]:
        B = F * S
        dev = torch.device("cuda", 0)
        # frame f of sequence s carries seeded instance (s + 131 f) mod 1024: every frame of a sequence has targets of its own
        fs = torch.arange(B, device=dev)
        idx = (fs % S + 131 * (fs // S)) % D
        payload = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)[idx].contiguous()
                   for a in (cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_offset, cons.ori_target, cons.ori_weight)]  # fmt: skip
        outs = lambda n: dict(error=torch.empty((n,), dtype=torch.float64, device=dev), iterations=torch.empty((n,), dtype=torch.int32, device=dev),
                              status=torch.empty((n,), dtype=torch.int32, device=dev))  # fmt: skip
        init = torch.from_numpy(th0).to(dev)[torch.arange(S, device=dev) % D].contiguous()
        # frames: one launch
        pf = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
        pf.set_constraints(*payload)
        pf.set_route("wave")
        thf, of = torch.zeros((F, S, P), dtype=torch.float32, device=dev), outs(B)

        def run_frames():
            thf[0].copy_(init)
            pf.solve_frames(thf, opt, F, outputs=of)

        # loop: the per-frame calls on one S-instance handle
        pl = capi.Problem(capi.RigHandle(rig, 0), S, cons.pos_parent, cons.ori_parent)
        pl.set_route("wave")
        thl, res, ol = torch.zeros((S, P), dtype=torch.float32, device=dev), torch.zeros((F, S, P), dtype=torch.float32, device=dev), outs(S)

        def run_loop():
            thl.copy_(init)
            for f in range(F):
                pl.set_constraints(*[a[f * S : (f + 1) * S] for a in payload])
                pl.solve(thl, opt, outputs=ol)
                res[f].copy_(thl)

        ways = {"frames": run_frames, "loop": run_loop}
        for run in ways.values():
            for _ in range(2):
                run()
        torch.cuda.synchronize()
        assert pf.last_route() == "wave" and pl.last_route() == "wave"
        assert torch.equal(thf, res), "solve_frames and the per-frame loop differ"
        it = of["iterations"].cpu().numpy()
        row = {"bit_identical": True, "iterations": {int(k): int(v) for k, v in sorted(Counter(int(x) for x in it).items())},
               "failed": int((of["status"].cpu().numpy() & 3 != 0).sum())}  # fmt: skip
        rates = {k: [] for k in ways}
        for _ in range(ROUNDS):
            for k, run in ways.items():
                rates[k].append(timed(run, B, WINDOW))
        for k in rates:
            r = np.array(rates[k])
            row[k] = dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()))
        lr = np.array(rates["loop"])
        row["loop_spread"] = float((lr.max() - lr.min()) / np.median(lr))
        row["frames_over_loop"] = row["frames"]["median"] / row["loop"]["median"]
        result["shapes"][f"{name} @ S={S} F={F}"] = row
        print(f"{name} @ S={S} F={F}: frames {row['frames']['median']:.3g} loop {row['loop']['median']:.3g} frames/s  x{row['frames_over_loop']:.2f}"
              f"  (loop spread {100 * row['loop_spread']:.1f} %)  mean iterations {it.mean():.2f}, max {it.max()}", flush=True)  # fmt: skip
        pf.close()
        pl.close()
        del payload, thf, res
        torch.cuda.empty_cache()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
