"""Closest points on a posed mesh: capi.Mesh.closest_points (mmx_closest_points_on_mesh, one kernel) against what a caller
writes without it -- the float32 broadcast of the same region form (Ericson 5.1.5 with torch.where, the distance from the
residual vector) plus argmin in torch on the device, chunked over the batch so that its [c, N, T] temporaries (about 30 are
alive at the peak) stay within 4 GiB (and over the sources where one instance exceeds that); the chunk sizes are recorded.
Same process, same seeded meshes and sources.

Shapes: the 72-joint humanoid's skinned torus (make_test_skinned_mesh 50 x 40: V = 2000, T = 4000) with N = 2000 sources at 256
and 4096 instances, and one large shared mesh (200 x 100: V = 20 000, T = 40 000, N = 20 000 at 16 instances).  The vertices are
the skinned vertices at random poses (momentum_amd.autograd.skin_points), the sources the tests' mix (on the surface and at
normal noise) around the surface at other poses.  The torch way is timed on the first TORCH_INSTANCES instances of the batch
(its chunks run one after the other, so its pairs/s does not depend on the batch size); the kernel on the whole batch.
The script records how far the two ways' distances are apart, and each way's largest distance error on the first instance against
the same torch code in float64 (the faces may differ where a source is equally near two faces; the posed meshes have slivers); it asserts the kernel's error.
Per shape the two alternate: two warm-up calls each, then five rounds each, every round timed with device events around at
least 0.3 s of calls.  Written per shape and way: median / min / max pairs/s (a pair = one source against one triangle), the
ratio of the medians, the round-to-round spread of either way, and the kernel's rate as a fraction of the issue roofline
    (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz) / (vector instructions per pair in the compiled loop: 53.3).
    python scripts/closest_points_on_mesh_rate.py [--out profiles/closest_points_on_mesh_rate.json] [--quick]
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
from momentum_amd import capi, make_humanoid72  # noqa: E402
from momentum_amd.rigs import make_test_skinned_mesh  # noqa: E402
from tests import closest_points_on_mesh_reference as cref  # noqa: E402
from tests import skeleton_state_reference as fk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_points_on_mesh_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small sizes (rehearsal); nothing is written")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 16  # distinct seeded poses, tiled over the batch
UNIT = 0.01  # bench.py's unit
LANE_OPS = 256 * 4 * 16 * 2.4e9  # vector lane-operations per second
INSTR_PER_PAIR = 852 / 16  # VALU instructions of the loop over four triangles x four sources (hipcc -O3, gfx950)
CHUNK_BYTES = 4 << 30
LIVE_TEMPORARIES = 30  # [c, N, T] float32 tensors alive at the peak of torch_way
TORCH_INSTANCES = 64


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


def torch_way(p, vtx, faces, chunk, source_chunk):
    """(face [B, N] int64, dist2 [B, N], barycentric [B, N, 3]) by the broadcast a caller writes; vtx may be [V, 3] (shared).
    `chunk` instances at a time and, within them, `source_chunk` sources at a time."""
    if source_chunk < p.shape[1]:
        parts = [torch_way(p[:, n : n + source_chunk], vtx, faces, chunk, p.shape[1]) for n in range(0, p.shape[1], source_chunk)]
        return tuple(torch.cat(x, 1) for x in zip(*parts))
    out = []
    dot = lambda u, w: (u * w).sum(-1)
    for b in range(0, p.shape[0], chunk):
        pb = p[b : b + chunk]
        vb = vtx[None] if vtx.dim() == 2 else vtx[b : b + chunk]
        a, bb, c = vb[:, faces[:, 0]], vb[:, faces[:, 1]], vb[:, faces[:, 2]]  # [c, T, 3]
        e1, e2 = (bb - a)[:, None], (c - a)[:, None]  # [c, 1, T, 3]
        d11, d12, d22 = dot(e1, e1), dot(e1, e2), dot(e2, e2)
        v = pb[:, :, None] - a[:, None]  # [c, N, T, 3]
        d1, d2 = dot(e1, v), dot(e2, v)
        d3, d4, d5, d6 = d1 - d11, d2 - d12, d1 - d12, d2 - d22
        vc, vb_, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1.0 / (va + vb_ + vc)
        s, t = vb_ * den, vc * den
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        m = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        s, t = torch.where(m, 1 - w, s), torch.where(m, w, t)
        m = (vb_ <= 0) & (d2 >= 0) & (d6 <= 0)
        s, t = torch.where(m, 0.0, s), torch.where(m, d2 / (d2 - d6), t)
        m = (d6 >= 0) & (d5 <= d6)
        s, t = torch.where(m, 0.0, s), torch.where(m, 1.0, t)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        s, t = torch.where(m, d1 / (d1 - d3), s), torch.where(m, 0.0, t)
        m = (d3 >= 0) & (d4 <= d3)
        s, t = torch.where(m, 1.0, s), torch.where(m, 0.0, t)
        m = (d1 <= 0) & (d2 <= 0)
        s, t = torch.where(m, 0.0, s), torch.where(m, 0.0, t)
        r = v - s[..., None] * e1 - t[..., None] * e2
        dist2 = dot(r, r)
        dist2 = torch.where(dist2 == dist2, dist2, torch.inf)  # (a degenerate face: NaN)
        best, face = dist2.min(-1)
        ws, wt = s.gather(-1, face[..., None])[..., 0], t.gather(-1, face[..., None])[..., 0]
        out.append((face, best, torch.stack([1 - ws - wt, ws, wt], -1)))
    return tuple(torch.cat(x) for x in zip(*out))


assert torch.cuda.is_available(), "closest_points_on_mesh_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "lane_operations_per_s": LANE_OPS, "unit": "pairs/s (one source point against one triangle)",
          "vector_instructions_per_pair": INSTR_PER_PAIR, "chunk_budget_bytes": CHUNK_BYTES, "torch_live_temporaries": LIVE_TEMPORARIES, "shapes": {}}  # fmt: skip
rig = make_humanoid72(seed=12345, variant="p128", unit=UNIT)
rh = capi.RigHandle(rig, 0)
for nu, nv, N, B, shared in [(50, 40, 2000, 256, False), (50, 40, 2000, 4096, False), (200, 100, 20000, 16, True)]:
    if args.quick:
        nu, nv, N, B = min(nu, 20), min(nv, 15), min(N, 300), min(B, 8)
    sk, tri = make_test_skinned_mesh(rig, nu, nv, 4, 12345)
    V, T = sk.rest.shape[0], tri.shape[0]
    skin = capi.Skin(rh, sk.joint, sk.weight, sk.inverse_bind, sk.rest)
    mesh = capi.Mesh(tri, V)
    pb = capi.Problem(rh, D, [0], [])
    idx = torch.arange(B, device=dev) % D
    pose = lambda seed: mauto.skin_points(skin, pb.skeleton_state(torch.from_numpy(np.ascontiguousarray(fk.random_inputs(rig, D, seed=seed)[0], np.float32)).to(dev)))
    posed = pose(1)
    vertices = posed[0].contiguous() if shared else posed[idx].contiguous()
    scale = float(np.abs(sk.rest).max())
    scan = cref.source_mix(pose(2).cpu().numpy(), tri, D, N, 7, noises=tuple(scale * x for x in cref.NOISES))
    source = torch.from_numpy(scan).to(dev)[idx].contiguous()
    faces = torch.from_numpy(tri.astype(np.int64)).to(dev)
    chunk = max(1, CHUNK_BYTES // (N * T * 4 * LIVE_TEMPORARIES))
    source_chunk = min(N, max(1, CHUNK_BYTES // (T * 4 * LIVE_TEMPORARIES)))  # (below N only where one instance exceeds the budget)
    Bt = min(B, TORCH_INSTANCES)
    got = {}

    def run_kernel():
        got["kernel"] = mesh.closest_points(source, vertices, float("inf"), want_barycentric=True, want_points=True, want_dist2=True)

    def run_torch():
        got["torch"] = torch_way(source[:Bt], vertices if shared else vertices[:Bt], faces, chunk, source_chunk)

    ways = {"closest_points_on_mesh_kernel": (run_kernel, B * N * T), "torch_region_form_argmin": (run_torch, Bt * N * T)}
    for run, _ in ways.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    kf, kd = got["kernel"][0][:Bt].long(), got["kernel"][3][:Bt]
    tf, td = got["torch"][0], got["torch"][1]
    differ = int((kf != tf).sum())
    gap = float((kd.sqrt() - td.sqrt()).abs().max())
    # the first instance against the same torch code in float64: whose distances are off where the two ways disagree
    exact = torch_way(source[:1].double(), (vertices if shared else vertices[:1]).double(), faces, 1, max(1, source_chunk // 2))[1].sqrt()
    err = {"kernel": float((kd[:1].sqrt().double() - exact).abs().max()), "torch": float((td[:1].sqrt().double() - exact).abs().max())}
    assert err["kernel"] <= 1e-4 * scale, (nu, nv, B, err, scale)
    row = {"batch": B, "N": N, "V": V, "T": T, "vertices_shared": shared, "torch_chunk_instances": chunk, "torch_chunk_sources": source_chunk, "torch_instances_timed": Bt,
           "plan": capi.closest_points_on_mesh_plan(B, N, T), "faces_differing_from_torch_way": differ, "largest_distance_gap_to_torch_way": gap,
           "largest_distance_error_against_float64_first_instance": err,
           "mesh_scale": scale}  # fmt: skip
    rates = {w: [] for w in ways}
    for _ in range(ROUNDS):
        for w, (run, pairs) in ways.items():
            rates[w].append(timed(run, pairs, WINDOW))
    for w in rates:
        row[w] = summary(rates[w])
    row["kernel_over_torch"] = row["closest_points_on_mesh_kernel"]["median"] / row["torch_region_form_argmin"]["median"]
    roof = LANE_OPS / INSTR_PER_PAIR
    row["issue_roofline_pairs_per_s"] = roof
    row["fraction_of_issue_roofline"] = row["closest_points_on_mesh_kernel"]["median"] / roof
    key = f"72-joint humanoid torus V={V} T={T} N={N} @ B={B}{' shared vertices' if shared else ''}"
    result["shapes"][key] = row
    print(f"{key}: kernel {row['closest_points_on_mesh_kernel']['median']:.4g} torch {row['torch_region_form_argmin']['median']:.4g} pairs/s  x{row['kernel_over_torch']:.1f}"
          f"  (spreads {100 * row['closest_points_on_mesh_kernel']['spread']:.1f} % / {100 * row['torch_region_form_argmin']['spread']:.1f} %; chunk {chunk}; {differ} faces differ,"
          f" distance gap {gap:.2e}, against float64 kernel {err['kernel']:.2e} torch {err['torch']:.2e}; {100 * row['fraction_of_issue_roofline']:.1f} % of the issue roofline)", flush=True)  # fmt: skip
    got.clear()
    skin.close(), mesh.close(), pb.close()
    del source, vertices, posed, faces
    torch.cuda.empty_cache()

if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
