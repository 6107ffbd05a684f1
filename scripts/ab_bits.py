"""Bit identity of two builds of the library in ONE process (loaded as scripts/ab_libs.py loads them): theta, iterations, status,
error_history and step_history of small solves -- a 3-joint and a 24-joint chain, B = 8, and the 72-joint humanoid, B = 64, for
the weak-damping and escalation cases -- on every route that accepts the case
(wave, one-launch, wide, explicit Jacobian; the double and mixed instantiations and MMX_PRECISION_AUTO through `precision`),
under every step rule and every do_line_search value, plus a weakly damped case (MMX_SOLVE_NOT_PD / DAMPING_FLOORED) and an
MMX_PRECISION_AUTO case whose elements escalate.  A combination a route refuses (MMX_ERR_UNSUPPORTED) must be refused by both.
Fails when a case differs, or when MMX_SOLVE_NOT_PD, DAMPING_FLOORED, PRECISION_SUSPECT, ESCALATED_F64 and MIXED were not all seen.
    python scripts/ab_bits.py --lib parent=<path to the other build's libmmx_hip.so> [--out file]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from momentum_amd import capi, humanoid72_landmark_joints, make_humanoid72, make_test_character  # noqa: E402
from momentum_amd._abi import GnOptions  # noqa: E402
from tests.helpers import make_problem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", required=True, metavar="NAME=PATH")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_rules_ab_bits.txt"))
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def load(path):
    capi._lib, capi.LIB_PATH = None, os.path.abspath(path)
    return capi.lib()


other_name, other_path = args.lib.split("=", 1)
LIBS = {other_name: load(other_path), "new": load(os.path.join(ROOT, "momentum_amd", "libmmx_hip.so"))}
ROUTES = ["wave", "fused", "wide", "explicit_jacobian"]
PRECISIONS = {"f32": 0, "f64": 1, "auto": 2, "mixed": 3}


def run(libname, rig, parents, cons, th0, route, opt):
    capi._lib = LIBS[libname]
    B = th0.shape[0]
    rh = capi.RigHandle(rig, 0)
    pb = capi.Problem(rh, B, parents, parents)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(pb.device)
        pb.set_constraints(t(cons.pos_offset), t(cons.pos_target), t(cons.pos_weight), t(cons.ori_offset), t(cons.ori_target), t(cons.ori_weight))
        pb.set_route(route)
        try:
            out = pb.solve(t(th0), opt, want_history=True, want_step_history=opt.step_rule == 1)
        except capi.MmxError as e:
            return f"refused ({e.code})", None
        torch.cuda.synchronize()
        return pb.last_route(), {k: v.cpu().numpy().copy() for k, v in out.items()}
    finally:
        pb.close()
        rh.close()


say(f"bit identity new / {other_name}: theta, error, iterations, status, error_history, step_history; device: {torch.cuda.get_device_name(0)}")
say(f"{'rig':>4} {'route':>17} {'prec':>5} {'rule':>4} {'ls':>2} {'lambda':>7}  ran as / status bits seen / identical")
bad, bits_seen = 0, set()
for J in (3, 24, 72):
    rig = make_test_character(J) if J < 72 else make_humanoid72(unit=0.01)
    parents = np.arange(J, dtype=np.int32) if J < 72 else humanoid72_landmark_joints(rig)
    cons, th0, _ = make_problem(rig, parents, parents, 8 if J < 72 else 64, seed=4242, perturb=0.3)
    cases = [(route, "f32", rule, ls, 0.05) for route in ROUTES for rule in (0, 1, 2) for ls in ((0, 1, 2) if rule == 0 else (0,))]
    cases += [("auto", prec, rule, ls, 0.05) for prec in ("f64", "mixed") for rule in (0, 1, 2) for ls in ((0, 1, 2) if rule == 0 else (0,))]
    cases += [(route, "f32", 0, 0, 1e-9) for route in ROUTES]  # weak damping: NOT_PD / DAMPING_FLOORED
    # MMX_PRECISION_AUTO with a bound nothing passes: every element escalates, to the mixed instantiation on the one-launch route,
    # to the double one where a route is pinned that has no mixed form (MMX_SOLVE_ESCALATED_F64)
    cases += [(route, "auto", rule, 0, 0.05) for route in ("auto", "wide", "explicit_jacobian") for rule in (0, 1)]
    if J == 72:  # undamped Gauss-Newton runs that meet non-positive pivots, in single precision and in double (MMX_SOLVE_NOT_PD)
        cases = cases[-6:] + [(route, prec, rule, 0, lam) for lam in (1e-5, 1e-7, 1e-12) for rule in (0, 1) for route, prec in [(r, "f32") for r in ROUTES[1:]] + [("auto", "f64")]]
    for route, prec, rule, ls, lam in cases:
        opt = GnOptions.make(min_iterations=2, max_iterations=12, threshold=10.0, regularization=lam, do_line_search=ls, step_rule=rule, precision=PRECISIONS[prec], precision_bound=1e-30 if prec == "auto" else 1e-5)
        ra, a = run(other_name, rig, parents, cons, th0, route, opt)
        rb, b = run("new", rig, parents, cons, th0, route, opt)
        if a is None or b is None:
            same = a is None and b is None and ra == rb
            seen = "-"
        else:
            same = ra == rb and set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
            seen = "|".join(str(s) for s in sorted(set(int(x) for x in b["status"])))
            bits_seen |= {bit for x in b["status"] for bit in (1, 2, 4, 8, 16, 32) if int(x) & bit}
        bad += 0 if same else 1
        say(f"{J:>4} {route:>17} {prec:>5} {rule:>4} {ls:>2} {lam:>7.0e}  {rb} / {seen} / {same}")
missing = {2, 4, 8, 16, 32} - bits_seen
say(f"{bad} differing cases; status bits seen {sorted(bits_seen)}, required and not seen {sorted(missing)}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad or missing else 0)
