"""Nearest-point queries: capi.closest_points (mmx_closest_points, one kernel) against what a caller writes without it -- the
float32 difference-form broadcast plus argmin in torch on the device,
    ((s[:, :, None] - t[:, None]) ** 2).sum(-1).argmin(-1)
(with normals: the pairs whose dot is below the threshold set to +inf first), chunked over the batch so that the [c, N, M, 3]
difference tensor stays within 4 GiB; the chunk size is recorded.  Same process, same seeded clouds.

Shapes: the 72-joint humanoid's skin (V = M = 2000) at 256 and 4096 instances; V = M = 20 000 at 16 instances with a shared
target; the 3-joint character (V = M = 500) at 4096 instances; each with and without normals.  Sources are the skinned vertices
at random poses (momentum_amd.autograd.skin_points), targets the vertices at other poses plus noise, normals random unit
vectors.  The script checks that the two ways agree on the index (they may differ at near-ties: the torch way has no fma).
Per shape the two alternate: two warm-up calls each, then five rounds each, every round timed with device events around at
least 0.3 s of calls.  Written per shape and way: median / min / max pairs/s (a pair = one source against one target), the
ratio of the medians, the round-to-round spread of either way; the kernel's rate as a fraction of the issue roofline
    (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz) / (vector instructions per pair in the steady-state loop's ISA: 6.5, 9.2 with normals);
and, without normals, the rate of the cdist form (torch.cdist(s, t).argmin(-1), chunked alike).  Last, on an offset cloud
(coordinates 100 +- 0.05, 4 x 2000 x 2000) the count of indices that are not the float64 argmin for the kernel, the torch
difference form and the cdist form.
    python scripts/closest_points_rate.py [--out profiles/closest_points_rate.json] [--quick]
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
from momentum_amd import capi, make_humanoid72, make_test_character, make_test_skin  # noqa: E402
from tests import closest_points_reference as cref  # noqa: E402
from tests import skeleton_state_reference as fk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_points_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small sizes (rehearsal); nothing is written")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 16  # distinct seeded poses, tiled over the batch
UNIT = 0.01  # bench.py's unit
LANE_OPS = 256 * 4 * 16 * 2.4e9  # vector lane-operations per second
INSTR_PER_PAIR = {False: 104 / 16, True: 147 / 16}  # VALU instructions of the loop over four targets x four sources (hipcc -O3, gfx950)
CHUNK_BYTES = 4 << 30
MIN_DOT = 0.25


def shapes():
    hum = make_humanoid72(seed=12345, variant="p128", unit=UNIT)
    return [("72-joint humanoid", hum, 2000, 256, False), ("72-joint humanoid", hum, 2000, 4096, False), ("72-joint humanoid", hum, 20000, 16, True),
            ("3-joint character", make_test_character(3), 500, 4096, False)]  # fmt: skip


def timed(run, count, seconds):
    """pairs/s over a window of at least `seconds` (device events around the whole window)"""
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


def summary(rates):
    r = np.array(rates)
    return dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()), spread=float((r.max() - r.min()) / np.median(r)))


def torch_way(s, t, ns, nt, chunk, form="difference"):
    """index [B, N] int64 by the broadcast a caller writes; t / nt may be [M, 3] (shared)"""
    out = []
    for b in range(0, s.shape[0], chunk):
        sb = s[b : b + chunk]
        tb = t[None] if t.dim() == 2 else t[b : b + chunk]
        if form == "cdist":
            d2 = torch.cdist(sb, tb.expand(sb.shape[0], -1, -1))
        else:
            d2 = ((sb[:, :, None] - tb[:, None]) ** 2).sum(-1)
        if ns is not None:
            ntb = nt[None] if nt.dim() == 2 else nt[b : b + chunk]
            d2 = torch.where((ns[b : b + chunk][:, :, None] * ntb[:, None]).sum(-1) >= MIN_DOT, d2, torch.inf)
        out.append(d2.argmin(-1))
    return torch.cat(out)


assert torch.cuda.is_available(), "closest_points_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "lane_operations_per_s": LANE_OPS, "unit": "pairs/s (one source point against one target point)",
          "vector_instructions_per_pair": {"plain": INSTR_PER_PAIR[False], "normals": INSTR_PER_PAIR[True]}, "chunk_budget_bytes": CHUNK_BYTES, "shapes": {}}  # fmt: skip
rng = np.random.default_rng(12345)
for name, rig, V, B, shared in shapes():
    if args.quick:
        B, V = min(B, 8), min(V, 700)
    s = make_test_skin(rig, V, 4, seed=12345)
    rh = capi.RigHandle(rig, 0)
    skin = capi.Skin(rh, s.joint, s.weight, s.inverse_bind, s.rest)
    pb = capi.Problem(rh, D, [0], [])
    idx = torch.arange(B, device=dev) % D
    pose = lambda seed: mauto.skin_points(skin, pb.skeleton_state(torch.from_numpy(np.ascontiguousarray(fk.random_inputs(rig, D, seed=seed)[0], np.float32)).to(dev)))
    source = pose(1)[idx].contiguous()
    scan = pose(2) + 0.02 * float(source.std()) * torch.from_numpy(rng.standard_normal((D, V, 3)).astype(np.float32)).to(dev)
    target = scan[0].contiguous() if shared else scan[idx].contiguous()
    sn = torch.from_numpy(cref.unit_normals(rng, (D, V))).to(dev)[idx].contiguous()
    tn_d = torch.from_numpy(cref.unit_normals(rng, (D, V))).to(dev)
    tn = tn_d[0].contiguous() if shared else tn_d[idx].contiguous()
    chunk = max(1, CHUNK_BYTES // (V * V * 12))
    pairs = B * V * V
    for normals in (False, True):
        a_sn, a_tn = (sn, tn) if normals else (None, None)
        got = {}

        def run_kernel():
            got["kernel"] = capi.closest_points(source, target, float("inf"), a_sn, a_tn, MIN_DOT, want_dist2=True, want_points=True)[0]

        def run_torch():
            got["torch"] = torch_way(source, target, a_sn, a_tn, chunk)

        def run_cdist():
            got["cdist"] = torch_way(source, target, None, None, chunk, "cdist")

        ways = {"closest_points_kernel": run_kernel, "torch_difference_argmin": run_torch}
        if not normals:
            ways["torch_cdist_argmin"] = run_cdist
        for run in ways.values():
            for _ in range(2):
                run()
        torch.cuda.synchronize()
        k, t = got["kernel"].long(), got["torch"]
        none = k < 0  # (with normals a source may have no eligible target; torch's argmin over all-inf rows says 0)
        differ = int(((k != t) & ~none).sum())
        assert differ <= 1e-3 * B * V, (name, V, B, normals, differ)
        row = {"batch": B, "N": V, "M": V, "target_shared": shared, "normals": normals, "torch_chunk_instances": chunk, "plan": capi.closest_points_plan(B, V, V, normals),
               "indices_differing_from_torch_way": differ, "sources_without_eligible_target": int(none.sum())}  # fmt: skip
        rates = {w: [] for w in ways}
        for _ in range(ROUNDS):
            for w, run in ways.items():
                rates[w].append(timed(run, pairs, WINDOW))
        for w in rates:
            row[w] = summary(rates[w])
        row["kernel_over_torch"] = row["closest_points_kernel"]["median"] / row["torch_difference_argmin"]["median"]
        roof = LANE_OPS / INSTR_PER_PAIR[normals]
        row["issue_roofline_pairs_per_s"] = roof
        row["fraction_of_issue_roofline"] = row["closest_points_kernel"]["median"] / roof
        key = f"{name} V=M={V} @ B={B}{' shared target' if shared else ''}{' with normals' if normals else ''}"
        result["shapes"][key] = row
        print(f"{key}: kernel {row['closest_points_kernel']['median']:.4g} torch {row['torch_difference_argmin']['median']:.4g} pairs/s  x{row['kernel_over_torch']:.1f}"
              f"  (spreads {100 * row['closest_points_kernel']['spread']:.1f} % / {100 * row['torch_difference_argmin']['spread']:.1f} %; chunk {chunk}; {differ} indices differ;"
              f" {100 * row['fraction_of_issue_roofline']:.1f} % of the issue roofline)" + ("" if normals else f"  cdist form {row['torch_cdist_argmin']['median']:.4g}"), flush=True)  # fmt: skip
        got.clear()
    skin.close(), pb.close()
    del source, scan, target, sn, tn, tn_d
    torch.cuda.empty_cache()

# ---- the offset cloud: who finds the float64 argmin
B, N, M = (2, 300, 300) if args.quick else (4, 2000, 2000)
c = cref.cloud("offset", B, N, M, 2024)
s, t = torch.from_numpy(c["source"]).to(dev), torch.from_numpy(c["target"]).to(dev)
exact = ((s.double()[:, :, None] - t.double()[:, None]) ** 2).sum(-1).argmin(-1)
wrong = {
    "closest_points_kernel": int((capi.closest_points(s, t)[0].long() != exact).sum()),
    "torch_difference_argmin": int((torch_way(s, t, None, None, B) != exact).sum()),
    "torch_cdist_argmin": int((torch_way(s, t, None, None, B, "cdist") != exact).sum()),
}
result["offset_cloud"] = {"coordinates": "100 +- 0.05", "batch": B, "N": N, "M": M, "sources": B * N, "indices_not_the_float64_argmin": wrong}
print("offset cloud, indices that are not the float64 argmin of", B * N, ":", wrong, flush=True)
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
