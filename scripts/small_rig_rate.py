"""Small rigs: the one-wavefront-per-instance route (MMX_ROUTE_WAVE) against the one-launch route (MMX_ROUTE_FUSED), same process,
same seeded device batch.

Per shape and batch size the two pinned routes alternate: two warm-up solves each, then five rounds each, every round timed
with device events around at least 0.3 s of solves.  Written per shape and route: median / min / max solves/s, the
fused-vs-fused spread of the five rounds, the worst rel of the first 1024 instances of that very batch against the oracle's
double run, the GPU iteration histogram.
    python scripts/small_rig_rate.py [--batches 4096,65536] [--out profiles/wave_route_rate.json] [--quick]
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
from oracle import oracle as orc  # noqa: E402
from tests.helpers import make_problem  # noqa: E402
from tests.test_real_rig import fixture_rig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="4096,65536")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_route_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, no oracle comparison (profiler runs)")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.05) if args.quick else (5, 0.3)
D = 1024  # distinct seeded instances, tiled to the batch

glb = fixture_rig(np.load(os.path.join(ROOT, "tests", "golden", "real_rig_character_with_motion.npz"), allow_pickle=True))
chain = make_test_character(24)
DRIVER = dict(min_iterations=4, max_iterations=50, threshold=10.0, regularization=0.01, do_line_search=2)
FIXED = dict(min_iterations=10, max_iterations=10, threshold=1.0, regularization=0.05)
SHAPES = [("glb driver defaults", glb, DRIVER), ("chain24 ten iterations lambda 0.05", chain, FIXED), ("chain24 driver defaults", chain, DRIVER)]


def timed(pb, th, th0d, opt, seconds):
    """solves/s over a window of at least `seconds` (device events around the whole window)"""
    n, done, ms = 1, 0, 0.0
    while ms < 1e3 * seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            th.copy_(th0d)
            pb.solve(th, opt)
        e1.record()
        e1.synchronize()
        ms, done = e0.elapsed_time(e1), n
        n *= 2
    return pb.B * done / (1e-3 * ms)


result = {"rounds": ROUNDS, "window_seconds": WINDOW, "shapes": {}}
for name, rig, okw in SHAPES:
    jj = np.arange(rig.num_joints, dtype=np.int32)
    cons, th0, _ = make_problem(rig, jj, jj, D, seed=12345, perturb=0.3)
    opt = GnOptions.make(**okw)
    ref = None if args.quick else orc.solve_batch(rig, cons, th0, opt, dtype="f64", nthreads=16)
    for B in [int(x) for x in args.batches.split(",")]:
        rep = lambda a: np.ascontiguousarray(np.tile(a, (B // D,) + (1,) * (a.ndim - 1)))
        pbs, row = {}, {}
        for route in ("fused", "wave"):
            pb = capi.Problem(capi.RigHandle(rig, 0), B, cons.pos_parent, cons.ori_parent)
            t = lambda a: torch.from_numpy(rep(np.asarray(a, np.float32))).to(pb.device)
            pb.set_constraints(t(cons.pos_offset), t(cons.pos_target), t(cons.pos_weight), t(cons.ori_offset), t(cons.ori_target), t(cons.ori_weight))
            pb.set_route(route)
            pbs[route] = pb
        th0d = torch.from_numpy(rep(th0)).to(pbs["fused"].device)
        th = th0d.clone()
        rates = {"fused": [], "wave": []}
        for route, pb in pbs.items():  # warm-up, and the answers of this very batch
            for _ in range(2):
                th.copy_(th0d)
                out = pb.solve(th, opt)
            torch.cuda.synchronize()
            assert pb.last_route() == route
            got = out["theta"][:D].cpu().numpy()
            it = out["iterations"].cpu().numpy()
            row[route] = {"iterations": {int(k): int(v) for k, v in sorted(Counter(int(x) for x in it).items())}}
            if ref is not None:
                rel = np.linalg.norm(got - ref["theta"], axis=1) / np.maximum(np.linalg.norm(ref["theta"], axis=1), 1e-3)
                row[route]["worst_rel_of_1024"] = float(rel.max())
        for _ in range(ROUNDS):
            for route, pb in pbs.items():
                rates[route].append(timed(pb, th, th0d, opt, WINDOW))
        for route in rates:
            r = np.array(rates[route])
            row[route].update(median=float(np.median(r)), min=float(r.min()), max=float(r.max()))
        fr = np.array(rates["fused"])
        row["fused_spread"] = float((fr.max() - fr.min()) / np.median(fr))
        row["wave_over_fused"] = row["wave"]["median"] / row["fused"]["median"]
        row["wave_beats_fused_by_more_than_the_spread"] = bool(row["wave"]["median"] > row["fused"]["median"] * (1.0 + row["fused_spread"]))
        result["shapes"][f"{name} @ {B}"] = row
        print(f"{name} @ {B}: fused {row['fused']['median']:.3g} wave {row['wave']['median']:.3g} solves/s  x{row['wave_over_fused']:.2f}"
              f"  (fused spread {100 * row['fused_spread']:.1f} %)  rel fused/wave {row['fused'].get('worst_rel_of_1024')} / {row['wave'].get('worst_rel_of_1024')}", flush=True)  # fmt: skip
        for pb in pbs.values():
            pb.close()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
