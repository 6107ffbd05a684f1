"""Gauss-Newton terms of vertex position constraints on every vertex of a skinned mesh with an instance's tiles divided over
`parts` workgroups (Problem.vertex_normal_equations(..., parts=...), mmx_skin_normal_equations_split) against parts = 1, the
one-workgroup-per-instance kernel of mmx_skin_normal_equations, in the same process on the same seeded parameters and targets.

Shapes: the 72-joint humanoid (p128: n = 128, K = 4) with V = C = 20 000 at 1 and 16 instances and V = C = 2 000 at 1, 16, 256
and 4096 instances.  Ways: parts 1, 2, 4, ... up to min(512, tiles), and "auto" (the library's plan for the shape); a way whose
workspace would exceed --max-workspace is left out and named; and min(auto, tiles // k) for k = 1, 2, 3, 4, 6, 8, 16 -- what the
library's plan would give if it kept at least k tiles per part: the sweep behind its rule that a part may be a single tile
(mmx_skin_normal_equations_plan.hpp; `auto` is asked of the library, so the sweep follows the plan's slots and LDS rule).
Per shape the ways alternate: warm-up calls, then five rounds each,
every round timed with device events around at least 0.3 s of calls (at least one call).  The workspace is allocated once per
way, outside the timed window.  Written per shape and way: median / min / max instances/s and constraint rows/s, the
round-to-round spread, and for auto its parts, its ratio to parts = 1 and the margin (the sum of the two spreads).

--kernels-only runs the 16-instance V = 20 000 shape at auto for a fixed number of calls and writes nothing: run it under a
kernel trace in a run of its own,
    rocprofv3 --kernel-trace -d <dir> -o sne -- python scripts/skin_normal_equations_split_rate.py --kernels-only
and then --merge-trace <dir>/sne_results.db (no GPU needed) reads the two kernels' durations from the trace's database and
writes them into --out as "kernels_at_V20000_B16_auto".  A later full run keeps that block.
    python scripts/skin_normal_equations_split_rate.py [--out profiles/skin_normal_equations_split_rate.json] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from momentum_amd import capi, make_humanoid72, make_test_skin  # noqa: E402
from tests import skeleton_state_reference as fk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_normal_equations_split_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small shapes (rehearsal); nothing is written")
ap.add_argument("--kernels-only", action="store_true", help="V = 20 000 at 16 instances, auto, 20 calls, nothing written (for a kernel trace)")
ap.add_argument("--merge-trace", metavar="DB", help="read the split kernel's and the reducer's durations from a rocprofv3 kernel-trace database into --out and exit")
ap.add_argument("--sweep-only", action="store_true", help="time parts = 1 and the parts of the tiles-per-part sweep only")
ap.add_argument("--max-workspace", type=float, default=2.0**31, help="bytes: ways that need more are left out")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 64  # distinct seeded instances, tiled over the batch
UNIT = 0.01  # bench.py's unit
SWEEP = (1, 2, 3, 4, 6, 8, 16)  # fewest tiles per part the plan could insist on (it insists on 1)
TRACE_KEY = "kernels_at_V20000_B16_auto"
SHAPES = [(20000, 1), (20000, 16), (2000, 1), (2000, 16), (2000, 256), (2000, 4096)]  # (V = C, instances)


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


if args.merge_trace:
    import sqlite3

    rows_ = sqlite3.connect(args.merge_trace).execute(
        "select name, count(*), avg(end - start), min(end - start), max(end - start), max(grid_x / workgroup_x) from kernels"
        " where name like '%skinNormalEquations%' group by name").fetchall()  # fmt: skip
    block = {"how": "rocprofv3 --kernel-trace of this script with --kernels-only, a run of its own; merged with --merge-trace"}
    for name, calls, mean, lo, hi, groups in rows_:
        key = "reduce_kernel_us" if "ReduceKernel" in name else ("split_kernel_us" if "<true>" in name else "unsplit_kernel_us")
        block[key] = dict(calls=calls, mean=mean / 1e3, min=lo / 1e3, max=hi / 1e3, workgroups=groups)
    assert "split_kernel_us" in block and "reduce_kernel_us" in block, rows_
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result[TRACE_KEY] = block
    json.dump(result, open(args.out, "w"), indent=1)
    print("merged", block, "into", args.out)
    sys.exit(0)
assert torch.cuda.is_available(), "skin_normal_equations_split_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
cus = torch.cuda.get_device_properties(0).multi_processor_count
rig = make_humanoid72(seed=12345, variant="p128", unit=UNIT)
rh = capi.RigHandle(rig, 0)
th0, _ = fk.random_inputs(rig, D, seed=12345)
th1, _ = fk.random_inputs(rig, D, seed=12346)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "compute_units": cus,
          "unit": "instances/s (one instance's H [n x n], g [n] and error of position constraints on all V vertices: 3 V rows); rows_per_s = 3 V x that",
          "yardstick": "parts = 1: the one-workgroup-per-instance kernel of mmx_skin_normal_equations, same process", "shapes": {}}  # fmt: skip
skins = {}
for V, B in [(20000, 16)] if args.kernels_only else SHAPES:
    if args.quick:
        B, V = min(B, 32), min(V, 500)
    if V not in skins:
        s = make_test_skin(rig, V, 4, seed=12345)
        skins[V] = capi.Skin(rh, s.joint, s.weight, s.inverse_bind, s.rest)
    skin = skins[V]
    pb = capi.Problem(rh, B, [0], [])
    pbD = capi.Problem(rh, D, [0], [])
    idx = torch.arange(B, device=dev) % D
    theta = torch.from_numpy(th0).to(dev)[idx].contiguous()
    target = skin.skin_points(pbD.skeleton_state(torch.from_numpy(th1).to(dev)))[idx].contiguous()
    rows = 3 * V
    tiles = -(-rows // 32)
    auto = pb.vertex_normal_equations_parts(skin, V, plane=False)
    if args.kernels_only:
        ws = torch.empty((max(capi.skin_normal_equations_workspace_bytes(B, pb.n, auto), 16),), dtype=torch.uint8, device=dev)
        for _ in range(20):
            pb.vertex_normal_equations(skin, theta, target, parts=auto, workspace=ws)
        torch.cuda.synchronize()
        print(f"kernels-only: V={V} B={B} parts={auto}: 20 calls done")
        sys.exit(0)
    ways, left_out = {}, []
    p = 1
    while p <= min(512, tiles):
        ways[f"parts_{p}"] = p
        p *= 2
    ways["auto"] = auto
    # the tiles-per-part sweep: the parts the plan would give if it kept at least k tiles per part -- the library's own answer
    # (slots, tiles and the cap) cut to tiles // k; a value already among the ways above is not timed twice
    sweep = {k: max(1, min(auto, tiles // k)) for k in SWEEP}
    for k, parts in sweep.items():
        if parts not in ways.values():
            ways[f"parts_{parts}"] = parts
    if args.sweep_only:
        ways = {k: v for k, v in ways.items() if v in sweep.values() or v == 1}
    runs, spaces = {}, {}
    for k, parts in list(ways.items()):
        need = capi.skin_normal_equations_workspace_bytes(B, pb.n, parts)
        if need > args.max_workspace:
            left_out.append(k)
            del ways[k]
            continue
        spaces[k] = torch.empty((need,), dtype=torch.uint8, device=dev) if need > 0 else None
        runs[k] = (lambda parts=parts, k=k: pb.vertex_normal_equations(skin, theta, target, parts=parts, workspace=spaces[k]))
    ref = runs["parts_1"]()
    torch.cuda.synchronize()
    for k, run in runs.items():  # warm-up, and the ways agree to the rounding of float32 sums in another association
        run()
        got = run()
        torch.cuda.synchronize()
        for a, b in zip(got, ref):
            d = float(((a.double() - b.double()).reshape(B, -1).abs().amax(1) / b.double().reshape(B, -1).abs().amax(1).clamp_min(1e-30)).max())
            assert d <= 1e-4, (V, B, k, d)
    rates = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, run in runs.items():
            rates[k].append(timed(run, B, WINDOW))
    row = {"batch": B, "V": V, "rows": rows, "tiles": tiles, "auto_parts": auto, "left_out_workspace_too_large": left_out, "ways": {}}
    for k in runs:
        row["ways"][k] = dict(parts=ways[k], workspace_bytes=0 if spaces[k] is None else int(spaces[k].numel()), ms_per_call=1e3 * B / float(np.median(rates[k])),
                              **summary(rates[k], rows))  # fmt: skip
    one, au = row["ways"]["parts_1"], row["ways"]["auto"]
    row["auto_over_parts_1"] = au["median"] / one["median"]
    row["margin"] = one["spread"] + au["spread"]
    best = max(runs, key=lambda k: row["ways"][k]["median"])
    row["best_way"] = best
    by_parts = {w["parts"]: w for w in row["ways"].values()}
    row["min_tiles_per_part_sweep"] = {str(k): dict(parts=parts, rows_per_s=by_parts[parts]["rows_per_s"], spread=by_parts[parts]["spread"])
                                       for k, parts in sweep.items() if parts in by_parts}  # fmt: skip
    result["shapes"][f"V={V} @ B={B}"] = row
    print(f"V={V} @ B={B} (T={tiles}): parts 1 {one['rows_per_s']:.4g} rows/s ({one['ms_per_call']:.3f} ms), auto = {auto} parts {au['rows_per_s']:.4g} rows/s"
          f" ({au['ms_per_call']:.3f} ms)  x{row['auto_over_parts_1']:.2f}  margin {100 * row['margin']:.1f} %; best {best} {row['ways'][best]['rows_per_s']:.4g} rows/s", flush=True)  # fmt: skip
    print("    " + "  ".join(f"{k}: {row['ways'][k]['rows_per_s']:.3g} ({100 * row['ways'][k]['spread']:.1f} %)" for k in runs), flush=True)
    print("    min tiles per part -> parts, rows/s: " + "  ".join(f"{k} -> {v['parts']}: {v['rows_per_s']:.3g}" for k, v in row["min_tiles_per_part_sweep"].items()), flush=True)
    pb.close(), pbD.close()
    del theta, target, spaces, runs
    torch.cuda.empty_cache()
for skin in skins.values():
    skin.close()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if os.path.exists(args.out):  # the kernel-trace block comes from another run (--merge-trace): keep it
        try:
            old = json.load(open(args.out))
            if TRACE_KEY in old:
                result[TRACE_KEY] = old[TRACE_KEY]
        except ValueError:
            pass
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
