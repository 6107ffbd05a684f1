"""A/B of whole LIBRARIES in ONE process on one GPU: this tree's libmmx_hip.so against other builds of it (the parent commit's
tree, a tree with one part of a change only), in the manner of ab_joint_pruning.py -- bench.py's device batches of cfg2 @ 4096,
cfg3 @ 65536 (LM schedule), cfg2 @ 4096 with the directional line search, and bench.py's two mixed-precision lines and its double
line, the libraries alternating.

Every library is loaded once (its own dlopen, its own handles; momentum_amd.capi is pointed at one or the other between the
windows).  Per shape: warm-up of every library, then THIS tree's library timed twice -- the spread of this process --, then
`--rounds` rounds over all libraries, every window `--steps` solves with a device synchronise inside the clock.  A library
counts as faster than the first one named (the baseline) when its median improvement exceeds twice the same-setting spread.
The results of all libraries are compared bit for bit as well.  With a second copy of the baseline's file named <baseline>2
(`--lib parent=a.so --lib parent2=copy_of_a.so`) the baseline-to-baseline spread is printed and this tree's library held to twice it.
    python scripts/ab_libs.py --lib parent=<path to the parent tree's libmmx_hip.so> [--lib name=path ...] [--shapes N] [--out file]
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
from momentum_amd import capi  # noqa: E402
from momentum_amd._abi import GnOptions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="another build of the library; the first one is the baseline")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--shapes", type=int, default=0, help="only the first N shapes (0: all)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_libs.txt"))
args = ap.parse_args()
assert args.steps >= 30 and args.rounds >= 3 and args.lib

# (name, config, B, step rule, line search, lambda, MMX_PRECISION_*, solves per window as a share of --steps)
SHAPES = [
    ("cfg2@4096", "cfg2", 4096, 0, 0, 0.05, 0, 1),
    ("cfg3@65536 (LM schedule)", "cfg3", 65536, 1, 0, 0.05, 0, 1),
    ("cfg2@4096 line search 2", "cfg2", 4096, 0, 2, 0.05, 0, 1),
    # bench.py's mixed-precision and double lines (the double kernel through mmx_solve's MMX_PRECISION_F64)
    ("cfg2@4096 lambda=1e-3 line search 2 mixed", "cfg2", 4096, 0, 2, 1e-3, 3, 1),
    ("cfg3@65536 mixed", "cfg3", 65536, 0, 0, 0.05, 3, 1),
    ("cfg2@4096 lambda=1e-5 line search 2 double", "cfg2", 4096, 0, 2, 1e-5, 1, 3),
]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def load(path):
    capi._lib, capi.LIB_PATH = None, os.path.abspath(path)
    return capi.lib()


LIBS = {name: load(path) for name, path in (a.split("=", 1) for a in args.lib)}
LIBS["new"] = load(os.path.join(ROOT, "momentum_amd", "libmmx_hip.so"))
BASE = next(iter(LIBS))


def use(name):
    capi._lib = LIBS[name]


def window(db, opt, steps):
    theta = db.theta0.clone()
    out = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        theta.copy_(db.theta0)
        out = db.pb.solve(theta, opt)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return db.B * steps / dt, out


say(f"library A/B, one process, {args.steps} solves per window, {args.rounds} rounds over {' / '.join(LIBS)}; device: {torch.cuda.get_device_name(0)}")
for name, cfg, B, rule, ls, lam, prec, share in SHAPES[: args.shapes or None]:
    steps = max(1, args.steps // share)
    rig, parents, _, _, _ = bench.build_rig(cfg)
    opt = GnOptions.make(min_iterations=10, max_iterations=10, threshold=1.0, regularization=lam, step_rule=rule, do_line_search=ls, precision=prec)
    dbs = {}
    for lib in LIBS:
        use(lib)
        dbs[lib] = bench.DeviceBatch(rig, parents, B, 0, 12345)
        window(dbs[lib], opt, args.warmup)
    use("new")
    same = [window(dbs["new"], opt, steps)[0] for _ in range(2)]
    spread = abs(same[0] - same[1]) / min(same)
    rates = {lib: [] for lib in LIBS}
    res = {}
    for _ in range(args.rounds):
        for lib in LIBS:
            use(lib)
            rate, out = window(dbs[lib], opt, steps)
            rates[lib].append(rate)
            res[lib] = {k: out[k].clone() for k in ("theta", "error", "iterations", "status")}
    say(f"{name}: route {dbs['new'].pb.last_route()}")
    say(f"  same library twice (new): {same[0]:.4e} {same[1]:.4e} solves/s, spread {100 * spread:.2f} %")
    med = {lib: statistics.median(r) for lib, r in rates.items()}
    for lib, r in rates.items():
        say(f"  {lib:>8}: " + " ".join(f"{x:.4e}" for x in r) + f"  median {med[lib]:.4e}")
    for lib in LIBS:
        if lib == BASE:
            continue
        gain = med[lib] / med[BASE] - 1.0
        equal = all(torch.equal(res[BASE][k], res[lib][k]) for k in res[lib])
        say(f"  {lib} / {BASE} - 1 = {100 * gain:+.2f} %   (twice the spread: {200 * spread:.2f} %; a gain: {gain > 2 * spread})   results bit-identical: {equal}")
    if BASE + "2" in LIBS:  # a second copy of the baseline's file: the baseline-to-baseline spread is the yardstick of a refactor
        both = rates[BASE] + rates[BASE + "2"]
        b2b = (max(both) - min(both)) / min(both)
        off = med["new"] / statistics.median(both) - 1.0
        say(f"  {BASE}-to-{BASE} spread (range of both copies' windows) {100 * b2b:.2f} %; new / median of them - 1 = {100 * off:+.2f} %; within twice the spread: {abs(off) <= 2 * b2b}")
    for lib in LIBS:  # (a handle is destroyed by the library that made it)
        use(lib)
        dbs[lib].pb.close()
        dbs[lib].rh.close()
    del dbs
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
