"""Forward + backward of a scalar loss of the skinned vertices: momentum_amd.autograd.skin_points (mmx_skin_points and
mmx_skin_points_backward: one kernel each) against what a caller writes without it -- the float32 torch gather-and-blend of
tests/skinning_reference.py on the device, differentiated by torch autograd (its backward scatters into the joints through
index_add) --, same process, same seeded states, the same loss L = sum(cotangent * vertices), gradient with respect to the state.

Shapes: the 72-joint humanoid with V = 2 000 and V = 20 000 (K = 4) at 256 and 4096 instances, the 3-joint character with
V = 500 at 4096 instances.  The script checks that the two results agree to single-precision rounding.  Per shape the two
alternate: two warm-up calls each, then five rounds each, every round timed with device events around at least 0.3 s of calls.
Written per shape and way: median / min / max evaluations/s (an evaluation = one instance's vertices and state gradient), the
ratio of the medians, the round-to-round spread of either way, the distance of the two results; and the forward kernel alone
(shared rest, and per-instance rest) as a fraction of the 8 TB/s HBM peak, its bytes being 12 B V written plus the state and
the per-instance rest when present.
    python scripts/skinning_rate.py [--out profiles/skinning_rate.json] [--quick]
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
from tests import skeleton_state_reference as fk  # noqa: E402
from tests import skinning_reference as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skinning_rate.json"))
ap.add_argument("--quick", action="store_true", help="one round, short windows, small batches (rehearsal); nothing is written")
args = ap.parse_args()
ROUNDS, WINDOW = (1, 0.02) if args.quick else (5, 0.3)
D = 256  # distinct seeded instances, tiled over the batch
UNIT = 0.01  # bench.py's unit
HBM_PEAK = 8e12  # bytes/s


def shapes():
    hum = make_humanoid72(seed=12345, variant="p128", unit=UNIT)
    out = [("72-joint humanoid", hum, V, 4, B) for V in (2000, 20000) for B in (256, 4096)]
    return out + [("3-joint character", make_test_character(3), 500, 4, 4096)]


def timed(run, count, seconds):
    """evaluations/s over a window of at least `seconds` (device events around the whole window)"""
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


assert torch.cuda.is_available(), "skinning_rate.py measures on the GPU"
dev = torch.device("cuda", 0)
result = {"rounds": ROUNDS, "window_seconds": WINDOW, "hbm_peak_bytes_per_s": HBM_PEAK,
          "unit": "evaluations/s (one instance's skinned vertices and the gradient of a scalar loss of them with respect to the state)", "shapes": {}}  # fmt: skip
for name, rig, V, K, B in shapes():
    if args.quick:
        B, V = min(B, 64), min(V, 2000)
    J = rig.num_joints
    s = make_test_skin(rig, V, K, seed=12345)
    rh = capi.RigHandle(rig, 0)
    skin = capi.Skin(rh, s.joint, s.weight, s.inverse_bind, s.rest)
    th0, _ = fk.random_inputs(rig, D, seed=12345)
    pb = capi.Problem(rh, D, [0], [])
    idx = torch.arange(B, device=dev) % D
    state = pb.skeleton_state(torch.from_numpy(th0).to(dev))[idx].contiguous().requires_grad_(True)
    cot = torch.from_numpy(np.random.default_rng(12346).normal(size=(D, V, 3)).astype(np.float32)).to(dev)[idx].contiguous()
    sk = ref.SkinTensors(s.joint, s.weight, s.inverse_bind, s.rest, J, torch.float32, dev)
    got = {}

    def run_kernels():
        state.grad = None
        v = mauto.skin_points(skin, state)
        (v * cot).sum().backward()
        got["kernels"] = (v.detach(), state.grad)

    def run_torch():
        state.grad = None
        v = ref.skin_points(sk, state)
        (v * cot).sum().backward()
        got["torch"] = (v.detach(), state.grad)

    ways = {"autograd_skin_points": run_kernels, "torch_gather_and_blend": run_torch}
    for run in ways.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    run_kernels(), run_torch()
    dist = []
    for a, b in zip(got["kernels"], got["torch"]):
        scale = b.reshape(B, -1).abs().amax(dim=1).clamp_min(1e-30)
        dist.append(float(((a - b).reshape(B, -1).abs().amax(dim=1) / scale).max()))
    assert max(dist) <= 1e-4, (name, V, B, dist)  # single-precision rounding of long float32 sums (the tests hold the real bound)
    entries = int((s.weight != 0).sum())
    row = {"batch": B, "J": J, "V": V, "K": K, "influences": entries, "max_rel_vertex_difference": dist[0], "max_rel_state_gradient_difference": dist[1]}
    got.clear()
    rates = {k: [] for k in ways}
    for _ in range(ROUNDS):
        for k, run in ways.items():
            rates[k].append(timed(run, B, WINDOW))
    for k in rates:
        row[k] = summary(rates[k])
    row["kernels_over_torch"] = row["autograd_skin_points"]["median"] / row["torch_gather_and_blend"]["median"]
    # the forward kernel alone against the HBM peak
    with torch.no_grad():
        st, out = state.detach(), torch.empty((B, V, 3), device=dev)
        rest_b = torch.from_numpy(s.rest).to(dev).unsqueeze(0).expand(B, -1, -1).contiguous()
        for key, rest, nbytes in (("forward_kernel_shared_rest", None, 12 * B * V + 32 * B * J), ("forward_kernel_instance_rest", rest_b, 24 * B * V + 32 * B * J)):
            run = lambda: skin.skin_points(st, rest, out=out)
            run(), torch.cuda.synchronize()
            f = summary([timed(run, B, WINDOW) for _ in range(ROUNDS)])
            f["bytes_per_call"] = nbytes
            f["fraction_of_hbm_peak"] = f["median"] / B * nbytes / HBM_PEAK
            row[key] = f
    result["shapes"][f"{name} V={V} @ B={B}"] = row
    print(f"{name} V={V} @ B={B}: autograd.skin_points {row['autograd_skin_points']['median']:.4g} torch gather-and-blend {row['torch_gather_and_blend']['median']:.4g} evaluations/s"
          f"  x{row['kernels_over_torch']:.2f}  (spreads {100 * row['autograd_skin_points']['spread']:.1f} % / {100 * row['torch_gather_and_blend']['spread']:.1f} %; vertices differ by {dist[0]:.1e},"
          f" state gradients by {dist[1]:.1e}); forward kernel alone {100 * row['forward_kernel_shared_rest']['fraction_of_hbm_peak']:.1f} % of the HBM peak,"
          f" {100 * row['forward_kernel_instance_rest']['fraction_of_hbm_peak']:.1f} % with per-instance rest", flush=True)  # fmt: skip
    skin.close(), pb.close()
    del state, cot, sk, rest_b, out, st
    torch.cuda.empty_cache()
if not args.quick:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print("wrote", args.out)
