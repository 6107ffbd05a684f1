"""Forward + backward of a scalar loss of the vertex normals: momentum_amd.autograd.vertex_normals (mmx_vertex_normals and
mmx_vertex_normals_backward: one kernel each, both gathers) against what a caller writes without it -- the float32 torch
gather / cross / index_add / normalise of tests/vertex_normals_reference.py on the device, differentiated by torch autograd
(its forward and backward scatter through index_add) --, same process, same posed vertices, the same loss
L = sum(cotangent * normals), gradient with respect to the positions.

Shapes: the make_test_skinned_mesh torus on the 72-joint humanoid, posed by mmx_skin_points at seeded states: 64 x 32
(V = 2 048) at 256 and 4096 instances, 200 x 100 (V = 20 000) at 16 and 256 instances.  The script records how far the two
results are apart.  Per shape the two alternate: two warm-up calls each, then five rounds each, every
round timed with device events around at least 0.3 s of calls.  Written per shape and way: median / min / max vertices/s (a
vertex = its normal and the gradient of a scalar loss with respect to its position), the ratio of the medians, the
round-to-round spread of either way, the distance of the two results; and the forward kernel alone (without and with the
sums) as a fraction of the 8 TB/s HBM peak over its algorithmic bytes, 24 B per vertex (12 read, 12 written; 36 B with sums).
    python scripts/vertex_normals_rate.py [--out profiles/vertex_normals_rate.json] [--quick]
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
from momentum_amd import capi, make_humanoid72, make_test_skinned_mesh  # noqa: E402
from tests import skeleton_state_reference as fk  # noqa: E402
from tests import vertex_normals_reference as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_normals_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small batches (rehearsal); nothing is written")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 16  # distinct seeded poses, tiled over the batch
UNIT = 0.01  # bench.py's unit
HBM_PEAK = 8e12  # bytes/s
SHAPES = [(64, 32, 256), (64, 32, 4096), (200, 100, 16), (200, 100, 256)]  # (nu, nv, instances)


def timed(run, count, seconds):
    """vertices/s over a window of at least `seconds` (device events around the whole window)"""
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


assert torch.cuda.is_available(), "vertex_normals_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
rig = make_humanoid72(seed=12345, variant="p128", unit=UNIT)
rh = capi.RigHandle(rig, 0)
pb = capi.Problem(rh, D, [0], [])
th0, _ = fk.random_inputs(rig, D, seed=12345)
states = pb.skeleton_state(torch.from_numpy(0.3 * th0).to(dev))  # (moderate poses: rotations within +-0.3 rad)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "hbm_peak_bytes_per_s": HBM_PEAK,
          "unit": "vertices/s (a vertex's normal and the gradient of a scalar loss of the normals with respect to its position)", "shapes": {}}  # fmt: skip
skins = {}
for nu, nv, B in SHAPES:
    if args.quick:
        B = min(B, 16)
    if (nu, nv) not in skins:
        skins[(nu, nv)] = make_test_skinned_mesh(rig, nu, nv, 4, seed=12345)
    s, tri_np = skins[(nu, nv)]
    V, T = s.rest.shape[0], tri_np.shape[0]
    skin = capi.Skin(rh, s.joint, s.weight, s.inverse_bind, s.rest)
    mesh = capi.Mesh(tri_np, V)
    idx = torch.arange(B, device=dev) % D
    pos = skin.skin_points(states)[idx].contiguous().requires_grad_(True)
    cot = torch.from_numpy(np.random.default_rng(12346).normal(size=(D, V, 3)).astype(np.float32)).to(dev)[idx].contiguous()
    tri = torch.from_numpy(tri_np.astype(np.int64)).to(dev)
    got = {}

    def run_kernels():
        pos.grad = None
        n = mauto.vertex_normals(mesh, pos)
        (n * cot).sum().backward()
        got["kernels"] = (n.detach(), pos.grad)

    def run_torch():
        pos.grad = None
        n = ref.vertex_normals(pos, tri)
        (n * cot).sum().backward()
        got["torch"] = (n.detach(), pos.grad)

    ways = {"autograd_vertex_normals": run_kernels, "torch_gather_and_index_add": run_torch}
    for run in ways.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    run_kernels(), run_torch()
    dist = []
    for a, b in zip(got["kernels"], got["torch"]):
        scale = b.reshape(B, -1).abs().amax(dim=1).clamp_min(1e-30)
        dist.append(float(((a - b).reshape(B, -1).abs().amax(dim=1) / scale).max()))
    # (recorded, not asserted: on a posed mesh that folds over itself a vertex sum nearly cancels and the float32 way loses that
    # vertex; tests/test_gpu_vertex_normals.py holds the real bound on meshes where float32 is sound)
    row = {"batch": B, "V": V, "T": T, "max_rel_normal_difference": dist[0], "max_rel_position_gradient_difference": dist[1]}
    got.clear()
    rates = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, run in ways.items():
            rates[k].append(timed(run, B * V, WINDOW))
    for k in rates:
        row[k] = summary(rates[k])
    row["kernels_over_torch"] = row["autograd_vertex_normals"]["median"] / row["torch_gather_and_index_add"]["median"]
    # the kernels alone; the forward against the HBM peak over its algorithmic bytes
    with torch.no_grad():
        p, out = pos.detach(), torch.empty((B, V, 3), device=dev)
        for key, sums, per_vertex in (("forward_kernel", False, 24), ("forward_kernel_with_sums", True, 36)):
            run = lambda: mesh.vertex_normals(p, want_sums=sums, out=out)
            run(), torch.cuda.synchronize()
            f = summary([timed(run, B * V, WINDOW) for _ in range(ROUNDS)])
            f["bytes_per_vertex"] = per_vertex
            f["fraction_of_hbm_peak"] = f["median"] * per_vertex / HBM_PEAK
            row[key] = f
        _, sm = mesh.vertex_normals(p, want_sums=True)
        run = lambda: mesh.vertex_normals_backward(p, sm, cot, out=out)
        run(), torch.cuda.synchronize()
        row["backward_kernel"] = summary([timed(run, B * V, WINDOW) for _ in range(ROUNDS)])
    result["shapes"][f"torus {nu}x{nv} V={V} @ B={B}"] = row
    print(f"V={V} @ B={B}: autograd.vertex_normals {row['autograd_vertex_normals']['median']:.4g} torch gather / index_add {row['torch_gather_and_index_add']['median']:.4g} vertices/s"
          f"  x{row['kernels_over_torch']:.2f}  (spreads {100 * row['autograd_vertex_normals']['spread']:.1f} % / {100 * row['torch_gather_and_index_add']['spread']:.1f} %; normals differ by {dist[0]:.1e},"
          f" position gradients by {dist[1]:.1e}); forward kernel alone {row['forward_kernel']['median']:.4g} vertices/s = {100 * row['forward_kernel']['fraction_of_hbm_peak']:.1f} % of the HBM peak,"
          f" {100 * row['forward_kernel_with_sums']['fraction_of_hbm_peak']:.1f} % with sums; backward kernel alone {row['backward_kernel']['median']:.4g} vertices/s", flush=True)  # fmt: skip
    skin.close(), mesh.close()
    del pos, cot, tri, out, p, sm
    torch.cuda.empty_cache()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
