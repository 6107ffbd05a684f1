"""mmx_eval_gradient on the shapes tests/test_gpu_eval_gradient.py does not have: random rigs, more than one pass of every
block-stride loop (U, n, J > 256), more than 512 solved parameters, one-sided and sparse constraint sets, every limit type,
per-instance pre-rotations, joint pruning on and off.

Reference and bound are that file's, unchanged (_check, _reference_of): per instance g64 = 2 J^T r and e64 from the oracle's
double evaluation, g32 / e32 from its float evaluation contracted in float32, and

    max|g - g64| <= 4 max(max|g32 - g64|, 2.5e-7 max|g64|)        |e - e64| <= 4 max(|e32 - e64|, 2.5e-7 e64)

with every instance away from the minimum (max|g64| > 1, e64 > 0: a condition on the inputs, checked for every instance).
Every test prints J, P, Kp, Ko, U, the enabled parameters, the non-zero columns of g64 and num_solve_joints of its case, then
_check's line per instance.

Which gap each group enters:
  random rigs (24)      rows of the parameter transform with three entries, translation / scale dofs on inner joints, non-zero
                        transform offsets, parameters shared across arbitrary joints (the extras loop over srcStart), stars and
                        bushy trees; Kp = 0 and Ko = 0; all five limit types; the prior; robust losses; a position,
                        orientation, limit or prior block switched off for one element; a random enabled mask
  rig300 dense          J = 300, U = 1200, n = 300: a second pass of the unit loop (loadUnitInput's other branch), of the
                        column loop and of the joint loops; nineteen 16-joint tiles in treeSumRanges / kRange; again with a
                        third of the parameters disabled; the two instances at positions 3 and 0 of a batch of five, bit-equal
  812 / 2048 parameters n > 512: slot tables from the max((n + 15) / 16, 1) branch, four and eight passes of the column loop
  rig300 sparse         Kp = 5, Ko = 0, U = 5 < J (the max(U, J) half of the LDS overlay), few loaded DFS positions, most
                        joints dead: joint_pruning on and off, bit-equal; the same pair on humanoid72
  chain24 pre-rotations per-instance translation offsets and pre-rotations, each instance against the oracle on its own rig

The inputs were checked with the oracle alone before the first GPU run (random rigs: smallest max|g64| 1.0045, smallest e64
0.475, largest float deviation 1.4e-6; rig300 dense max|g64| 165 / 97.7; 812 parameters 156 / 271; 2048 parameters 90.9) and
where the recipe left a choice:
  rig300 sparse                  perturb = 0.5, offsets of up to 3 cm: max|g64| 2.65 / 5.86, e64 0.597 / 2.26.  (With the points AT
                                 their joints' origins that joint's own rotation columns are exact zeros of the oracle by
                                 cancellation, not by structure; the kernel's N - t x F leaves 1.4e-9 of max|g| there.)
  rig300 dense, a third disabled max|g64| 141 / 83.1
  chain24 pre-rotations          max|g64| 5586 / 3452 / 7527

Found by the random rigs (seeds 4 and 16): a MINMAX_JOINT / LINEAR_JOINT row of the oracle's (and mmx_eval_jacobian's) J has
entries in DISABLED columns -- the reference implementation scatters the whole transform row and its solver drops the columns
afterwards -- so 2 J^T r of the raw J is non-zero at a disabled parameter, where mmx_eval_gradient promises an exact zero.
The reference of the random rigs is therefore taken over the enabled columns (_fuzz_reference, which also asserts that those
rows are the only entries this removes); include/mmx.h now says so.

Deviations the MI355X reaches: per group the instance that comes closest to its bound as the share of the bound it uses, then
that instance's figure relative to max|g64| / e64 with the bound in brackets (measured once with this file's inputs):
  random rigs (72 instances)     gradient 0.39: 3.94e-07 (1.00e-06)   error 0.40: 3.95e-07 (1.00e-06)
  rig300_dense                   gradient 0.35: 3.85e-07 (1.10e-06)   error 0.15: 1.50e-07 (1.00e-06)
  rig300_dense_third_disabled    gradient 0.29: 3.74e-07 (1.28e-06)   error 0.15: 1.50e-07 (1.00e-06)
  p812                           gradient 0.40: 5.36e-07 (1.33e-06)   error 0.16: 1.56e-07 (1.00e-06)
  p812 vs eval_jacobian          gradient 0.42: 5.52e-07 (1.33e-06)   error 0.10: 1.01e-07 (1.00e-06)
  p2048                          gradient 0.35: 3.52e-07 (1.00e-06)   error 0.01: 9.83e-09 (1.00e-06)
  p2048 vs eval_jacobian         gradient 0.44: 4.44e-07 (1.00e-06)   error 0.11: 1.13e-07 (1.00e-06)
  rig300_sparse (both settings)  gradient 0.07: 7.28e-08 (1.00e-06)   error 0.10: 9.99e-08 (1.00e-06)
  humanoid72 (both settings)     gradient 0.20: 3.17e-07 (1.59e-06)   error 0.08: 7.82e-08 (1.01e-06)
  chain24_pre_rotations          gradient 0.23: 3.09e-07 (1.32e-06)   error 0.17: 1.94e-07 (1.13e-06)
num_solve_joints: rig300_sparse 29 of 300, humanoid72 41 of 72 with pruning; all joints without.
"""
import functools

import numpy as np
import pytest

from momentum_amd import make_rig300, make_test_character
from momentum_amd._abi import MMX_LIMIT_LINEAR_JOINT, MMX_LIMIT_MINMAX_JOINT, MMX_LOSS_WELSCH, ParameterLimit
from tests.helpers import make_problem
from tests.test_gpu_eval_gradient import _case, _check, _eval, _problem, _reference, _reference_of, _with
from tests.test_gpu_fuzz import random_rig
from tests.test_gpu_many_parameters import _every_joint_dof_rig, _many_parameter_rig
from tests.test_gpu_per_instance import _variants

pytestmark = pytest.mark.gpu
FUZZ_SEEDS = 24
SPARSE_PERTURB = 0.5


# ---------------------------------------------------------------------------------------------------------------------
# cases (dicts of tests/test_gpu_eval_gradient._case's layout; "inst_rig": per-instance (offsets, pre-rotations) or absent)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fuzz_case(seed):
    from oracle import oracle as orc

    B = 3
    rng = np.random.default_rng(21000 + seed)
    J = int(rng.integers(2, 48))
    rig = random_rig(rng, J, ["chain", "star", "bushy"][seed % 3])
    P = rig.num_params
    Kp, Ko = int(rng.integers(1, 9)), int(rng.integers(1, 6))
    if seed % 4 == 1:
        Ko = 0
    if seed % 4 == 2:
        Kp = 0
    pp = rng.integers(0, J, size=Kp).astype(np.int32)
    op = rng.integers(0, J, size=Ko).astype(np.int32)
    cons, _, _ = make_problem(rig, pp, op, B, seed=seed, perturb=0.25, random_offsets=True, weights="random")
    en = (rng.uniform(size=P) < 0.8).astype(np.uint8)
    en[:3] = 1
    theta = rng.uniform(-0.3, 0.3, size=(B, P)).astype(np.float32)
    a, b2, c3 = (int(x) for x in rng.choice(P, size=3, replace=False))
    limits = [ParameterLimit.minmax(a, -0.05, 0.05, 1.5), ParameterLimit.linear(a, b2, 0.7, 0.02), ParameterLimit.halfplane(b2, c3, 0.6, 0.8, 0.1, 1.2)]
    rows = [r for r in range(7 * J) if rig.pt_outer[r + 1] - rig.pt_outer[r] in (1, 2)]
    r0 = int(rng.choice(rows))
    limits.append(ParameterLimit.minmax_joint(r0 // 7, r0 % 7, -0.02, 0.03, 1.0))
    if len(rows) >= 2:
        r1, r2 = (int(x) for x in rng.choice(rows, size=2, replace=False))
        limits.append(ParameterLimit.linear_joint(r1 // 7, r1 % 7, r2 // 7, r2 % 7, 0.8, 0.01))
    kw = dict(limits=limits, limit_function_weight=0.5)
    if seed % 2 == 0:
        kw.update(model_target=rng.uniform(-0.2, 0.2, size=(B, P)).astype(np.float32),
                  model_weights=rng.uniform(-0.3, 1.0, size=(B, P)).astype(np.float32), model_function_weight=0.8)  # fmt: skip
    if seed % 3 == 1:
        kw.update(pos_loss=(1.0, 0.5), ori_loss=(0.0, 1.0))
    if seed % 3 == 2:
        kw.update(pos_loss=(MMX_LOSS_WELSCH, 1.5), ori_loss=(MMX_LOSS_WELSCH, 1.0))
    fw = rng.uniform(0.5, 1.5, size=(B, 4)).astype(np.float32)
    fw[1, seed % 4] = 0.0  # element 1: the position (seeds 0, 4, ...), orientation, limit or prior block off
    full = orc.Constraints(cons.pos_parent, cons.pos_offset, cons.pos_target, cons.pos_weight, cons.ori_parent, cons.ori_offset, cons.ori_target,
                           cons.ori_weight, pos_function_weight=0.9, ori_function_weight=1.1, function_weights=fw, **kw)  # fmt: skip
    return dict(rig=rig, rigs=[rig] * B, cons=full, theta=theta, enabled=en, offsets=None, B=B)


def _every_joint(rig, B, **kw):
    jj = np.arange(rig.num_joints, dtype=np.int32)
    cons, th0, _ = make_problem(rig, jj, jj, B, **kw)
    return dict(rig=rig, rigs=[rig] * B, cons=cons, theta=th0, enabled=None, offsets=None, B=B)


@functools.lru_cache(maxsize=None)
def _big_case(name):
    if name in ("rig300_dense", "rig300_dense_third_disabled"):  # J = 300, U = 1200, n = 300
        c = _every_joint(make_rig300(unit=0.01), 2, seed=77, perturb=0.1)
        if name.endswith("disabled"):
            c["enabled"] = np.ones(c["rig"].num_params, np.uint8)
            c["enabled"][1::3] = 0
        return c
    if name == "p812":
        return _every_joint(_many_parameter_rig(3), 2, seed=77, perturb=0.1)
    if name == "p2048":  # a translation, rotation and scale column on nearly every joint
        return _every_joint(_every_joint_dof_rig(skip=[40 * i + 6 for i in range(52)]), 1, seed=79, perturb=0.03, random_offsets=True, offset_scale=0.03)
    if name == "rig300_sparse":  # five position constraints, deep in the tree; no orientation block
        rig, B = make_rig300(unit=0.01), 2
        deep = [j for j, d in enumerate(rig.depth()) if d >= 12][-5:]
        # (offsets of a few centimetres: with a point AT its joint's origin the joint's own rotation columns are exact zeros of the
        # oracle by cancellation, not by structure -- the kernel's N - t x F leaves 1e-9 of max|g| there, inside the bound)
        cons, th0, _ = make_problem(rig, deep, [], B, seed=77, perturb=SPARSE_PERTURB, random_offsets=True, offset_scale=0.03)
        return dict(rig=rig, rigs=[rig] * B, cons=cons, theta=th0, enabled=None, offsets=None, B=B)
    assert name == "chain24_pre_rotations"
    rig, B = make_test_character(24), 3
    jj = list(range(24))
    cons, th0, _ = make_problem(rig, jj, jj, B, seed=12345, perturb=0.3, random_offsets=True, weights="random", theta0_scale=0.2)
    off, pre, rigs = _variants(rig, B, np.random.default_rng(31), scale=0.1)
    return dict(rig=rig, rigs=rigs, cons=cons, theta=th0, enabled=None, offsets=None, inst_rig=(off, pre), B=B)


@functools.lru_cache(maxsize=None)
def _big_reference(name):
    return _reference_of(_big_case(name))


@functools.lru_cache(maxsize=None)
def _fuzz_reference(seed):
    """_reference_of the case, over the enabled parameters.  The oracle's J is the reference implementation's: a row of a
    joint-parameter limit (MINMAX_JOINT, LINEAR_JOINT) carries every column of its transform row, enabled or not, and the
    solver drops the disabled columns afterwards.  mmx_eval_gradient is defined over what a solve sees -- exact zeros at
    disabled parameters (include/mmx.h) -- so g64 / g32 are set to zero there.  That these rows are the ONLY entries removed
    is asserted: without the joint-parameter limits the oracle's gradient is exactly zero at every disabled parameter."""
    from oracle import oracle as orc

    c = _fuzz_case(seed)
    off = c["enabled"] == 0
    plain = dict(c, cons=_with(c["cons"], orc, limits=[lm for lm in c["cons"].limits if lm.type not in (MMX_LIMIT_MINMAX_JOINT, MMX_LIMIT_LINEAR_JOINT)]))
    g64p, _, g32p, _ = _reference_of(plain)
    assert len(plain["cons"].limits) == 3 and np.all(g64p[:, off] == 0.0) and np.all(g32p[:, off] == 0.0)
    g64, e64, g32, e32 = _reference_of(c)
    g64, g32 = np.where(off[None], 0.0, g64), np.where(off[None], np.float32(0.0), g32)
    for a in (g64, g32):
        a.setflags(write=False)
    return g64, e64, g32, e32


# ---------------------------------------------------------------------------------------------------------------------
def _make(tag, c, ref, pruning=True):
    """The case's problem; prints the shape figures a reader needs to see which loops and tables the case enters."""
    pb = _problem(c)
    if c.get("inst_rig") is not None:
        pb.set_instance_rig(*c["inst_rig"])
    if not pruning:
        pb.set_joint_pruning(False)
    cons, rig = c["cons"], c["rig"]
    print(f"\n{tag}: J {rig.num_joints} P {rig.num_params} Kp {cons.Kp} Ko {cons.Ko} U {cons.Kp + 3 * cons.Ko} enabled (n at most) {pb.n} "
          f"non-zero columns of g64 (n at least) {int((ref[0] != 0.0).any(axis=0).sum())} num_solve_joints {pb.num_solve_joints()}")  # fmt: skip
    return pb


def _assert_gradient(tag, c, g, e, ref):
    B, P = c["B"], c["rig"].num_params
    assert g.shape == (B, P) and g.dtype == np.float32 and e.shape == (B,) and e.dtype == np.float64
    _check(tag, g, e, ref)
    if c["enabled"] is not None:
        off = c["enabled"] == 0
        assert np.all(g[:, off] == 0.0) and not np.signbit(g[:, off]).any()  # exact +0.0
    assert np.all(g[ref[0] == 0.0] == 0.0)  # structurally zero columns, rows of switched-off blocks


def _assert_forms_agree(torch, pb, theta, g, e):
    g_only, none_e = _eval(torch, pb, theta, want_err=False)
    none_g, e_only = _eval(torch, pb, theta, want_grad=False)
    assert none_e is None and none_g is None
    assert np.array_equal(g_only, g) and np.array_equal(e_only, e)


def _jacobian_reference(torch, pb, theta, ref):
    """2 J^T r of the handle's own mmx_eval_jacobian contracted in float64, with the oracle's float deviation around it
    (test_gradient_matches_the_handles_own_jacobian of tests/test_gpu_eval_gradient.py)."""
    jac, res, err = pb.eval_jacobian(torch.from_numpy(theta).to(pb.device))
    torch.cuda.synchronize()
    gj = 2.0 * np.einsum("bpm,bm->bp", jac.cpu().numpy().astype(np.float64), res.cpu().numpy().astype(np.float64))
    ej = err.cpu().numpy()
    g64, e64, g32, e32 = ref
    return gj, ej, gj + (g32.astype(np.float64) - g64), ej + (e32 - e64)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_random_rig_holds_the_oracle_bound(torch_cuda, seed):
    torch = torch_cuda
    c = _fuzz_case(seed)
    ref = _fuzz_reference(seed)
    tag = f"random rig {seed}"
    pb = _make(tag, c, ref)
    g, e = _eval(torch, pb, c["theta"])
    _assert_gradient(tag, c, g, e, ref)
    if seed < 4:  # one of each constraint-set shape: both blocks, positions only, orientations only, both
        _assert_forms_agree(torch, pb, c["theta"], g, e)
    jac, res, err = pb.eval_jacobian(torch.from_numpy(c["theta"]).to(pb.device))  # the Jacobian path takes the same problem
    torch.cuda.synchronize()
    assert pb.M == c["cons"].rows and tuple(jac.shape) == (c["B"], c["rig"].num_params, pb.M)


@pytest.mark.parametrize("name", ["rig300_dense", "rig300_dense_third_disabled"])
def test_past_one_pass_of_every_loop(torch_cuda, name):
    torch = torch_cuda
    c, ref = _big_case(name), _big_reference(name)
    assert c["rig"].num_joints > 256 and c["rig"].num_params > 256 and c["cons"].Kp + 3 * c["cons"].Ko > 4 * 256
    pb = _make(name, c, ref)
    g, e = _eval(torch, pb, c["theta"])
    _assert_gradient(name, c, g, e, ref)
    if name == "rig300_dense_third_disabled":
        assert int((c["enabled"] == 0).sum()) == 100
        return
    _assert_forms_agree(torch, pb, c["theta"], g, e)
    pb.eval_jacobian(torch.from_numpy(c["theta"]).to(pb.device))
    torch.cuda.synchronize()
    # the two instances at positions 3 and 0 of a batch of five, other instances around them
    where, BB = [3, 0], 5
    rig, cons = c["rig"], c["cons"]
    jj = np.arange(rig.num_joints, dtype=np.int32)
    big, thb, _ = make_problem(rig, jj, jj, BB, seed=177, perturb=0.1)
    theta = thb.copy()
    for b, w in enumerate(where):
        for k in ("pos_offset", "pos_target", "pos_weight", "ori_offset", "ori_target", "ori_weight"):
            getattr(big, k)[w] = getattr(cons, k)[b]
        theta[w] = c["theta"][b]
    g5, e5 = _eval(torch, _problem(c, BB, big), theta)
    assert np.array_equal(g5[where], g) and np.array_equal(e5[where], e)
    assert not np.array_equal(g5[1], g[0])  # (the instances around them are other problems)


@pytest.mark.parametrize("name", ["p812", "p2048"])
def test_beyond_512_solved_parameters(torch_cuda, name):
    """Inside the LDS budget (about 100 KB and 110 KB of 160 KB), so the call is accepted: a refusal raises here."""
    torch = torch_cuda
    c, ref = _big_case(name), _big_reference(name)
    pb = _make(name, c, ref)
    assert pb.n == c["rig"].num_params == int(name[1:]) and pb.n > 512
    g, e = _eval(torch, pb, c["theta"])
    _assert_gradient(name, c, g, e, ref)
    assert int((ref[0] != 0.0).any(axis=0).sum()) == pb.n  # every column is solved: the kernel's n is pb.n
    _check(name + " vs eval_jacobian", g, e, _jacobian_reference(torch, pb, c["theta"], ref))


@pytest.mark.parametrize("name", ["rig300_sparse", "humanoid72"])
def test_joint_pruning_on_and_off_is_bit_equal(torch_cuda, name):
    torch = torch_cuda
    c, ref = (_case(name), _reference(name)) if name == "humanoid72" else (_big_case(name), _big_reference(name))
    J = c["rig"].num_joints
    if name == "rig300_sparse":
        assert c["cons"].Ko == 0 and c["cons"].Kp == 5 < J
    got = {}
    for pruning in (True, False):
        tag = f"{name} joint_pruning {'default' if pruning else '-1'}"
        pb = _make(tag, c, ref, pruning)
        assert pb.num_solve_joints() < J if pruning else pb.num_solve_joints() == J
        got[pruning] = _eval(torch, pb, c["theta"])
        _assert_gradient(tag, c, *got[pruning], ref)
    assert np.array_equal(got[True][0], got[False][0]) and np.array_equal(got[True][1], got[False][1])


def test_per_instance_pre_rotations(torch_cuda):
    torch = torch_cuda
    name = "chain24_pre_rotations"
    c, ref = _big_case(name), _big_reference(name)
    off, pre = c["inst_rig"]
    assert np.abs(pre[1] - pre[0]).max() > 0.05 and np.abs(off[1] - off[0]).max() > 0.0
    pb = _make(name, c, ref)
    g, e = _eval(torch, pb, c["theta"])
    _assert_gradient(name, c, g, e, ref)
