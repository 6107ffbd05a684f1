"""CPU checks of the joint-to-joint distance block (include/mmx.h, MMX_JC_JOINT_TO_JOINT_DISTANCE): the header constant
against its mirror with the ABI unchanged, the double reference's analytic rows against central differences on both
recipes, the float32 replay of the reference against its double run (the precondition of the GPU test of the
single-precision routes), the JointBlock marshalling and the solver2 class."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from momentum_amd import _abi, make_test_character, solver2
from tests import joint_pair_reference as jp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_BLOCK_SIZE = 88  # sizeof(mmx_joint_constraint_block) of the commit before this type (ABI 12, LP64)


def test_header_constant_matches_the_mirror_and_the_abi_is_unchanged():
    prog = r"""
    #include <stdio.h>
    #include "mmx.h"
    int main(void) {
      printf("%d %d %zu %d\n", MMX_JC_JOINT_TO_JOINT_DISTANCE, MMX_ABI_VERSION, sizeof(mmx_joint_constraint_block), MMX_MAX_JOINT_BLOCKS);
      return 0;
    }"""
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == [_abi.MMX_JC_JOINT_TO_JOINT_DISTANCE, 12, PARENT_BLOCK_SIZE, _abi.MMX_MAX_JOINT_BLOCKS]
    assert _abi.MMX_JC_JOINT_TO_JOINT_DISTANCE == 10 and _abi.MMX_ABI_VERSION == 12
    assert C.sizeof(_abi.JointConstraintBlock) == PARENT_BLOCK_SIZE
    assert _abi.jc_func_dim(_abi.MMX_JC_JOINT_TO_JOINT_DISTANCE) == 1
    assert "wave" in _abi.ROUTES and len(_abi.ROUTES) == 5  # no route value was added


def _fd_check(rig, blk, theta, h=1e-6):
    """analytic pair rows against central differences of the residual; returns the worst difference over max|J|"""
    J, r, e = jp.pair_rows(rig, blk, theta)
    assert abs(r @ r - e) <= 1e-9 * max(1.0, e)
    worst = 0.0
    for p in range(rig.num_params):
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        fd = (jp.pair_rows(rig, blk, tp)[1] - jp.pair_rows(rig, blk, tm)[1]) / (2 * h)
        worst = max(worst, np.abs(fd - J[:, p]).max())
    return worst / np.abs(J).max(), J


def test_reference_rows_match_central_differences_on_the_humanoid():
    rig, base, blocks, th0, ths = jp.recipe_h(64)
    for b, theta in ((0, th0[0]), (1, ths[1]), (63, 0.5 * ths[63])):
        err, _ = _fd_check(rig, blocks[0].instance(b), theta.astype(np.float64))
        print(f"recipe H element {b}: analytic - central difference = {err:.2e} max|J|")
        assert err <= 1e-6, (b, err)


@pytest.mark.parametrize("which", range(3))
def test_reference_rows_match_central_differences_on_the_small_rigs(which):
    rig, base, blocks, th0, ths = jp.recipe_s(which, 16)
    J = blocks[0].count
    assert J == {0: 55, 1: 55, 2: 21}[which]
    assert float(blocks[0].plane_d.min()) > 1e-2  # no pair of points (same-joint pairs included) is near coincidence
    for b, theta in ((0, th0[0]), (15, ths[15])):
        err, _ = _fd_check(rig, blocks[0].instance(b), theta.astype(np.float64))
        print(f"recipe S rig {which} element {b}: analytic - central difference = {err:.2e} max|J|")
        assert err <= 1e-6, (which, b, err)


def test_pair_rows_reach_columns_the_anchor_rows_do_not():
    rig, base, blocks, th0, _ = jp.recipe_h(64)
    J, _, _ = jp.full_rows(rig, base.instance(0), [blocks[0].instance(0)], th0[0])
    split = 3 * base.Kp
    anchor = np.abs(J[:split]).max(axis=0) > 0
    pair = np.abs(J[split:split + blocks[0].count]).max(axis=0) > 0
    print(f"columns: pair rows {int(pair.sum())}, anchor rows {int(anchor.sum())}, pair only {int((pair & ~anchor).sum())} of {J.shape[1]}")
    assert int((pair & ~anchor).sum()) >= 50


def _objective_ratio(recipe, solved):
    rig, base, blocks, th0, _ = recipe
    out = []
    for b in range(th0.shape[0]):
        inst = (base.instance(b), [k.instance(b) for k in blocks])
        out.append(jp.full_rows(rig, *inst, solved[b])[2] / jp.full_rows(rig, *inst, th0[b])[2])
    return np.array(out)


def test_float32_replay_stays_within_1e5_of_the_double_run_on_the_humanoid():
    B = 64
    d = jp.rel(jp.solved_h(B, True).astype(np.float64), jp.solved_h(B))
    ratio = _objective_ratio(jp.recipe_h(B), jp.solved_h(B))
    print(f"recipe H: float32 replay vs double, worst of {B}: {d.max():.2e}; objective after / before, worst: {ratio.max():.2e}")
    assert d.max() <= 1e-5, d
    assert ratio.max() <= 1e-2, ratio  # the double run converges on every element


@pytest.mark.parametrize("which", range(3))
def test_float32_replay_stays_within_1e5_of_the_double_run_on_the_small_rigs(which):
    B = 16
    d = jp.rel(jp.solved_s(which, B, True).astype(np.float64), jp.solved_s(which, B))
    ratio = _objective_ratio(jp.recipe_s(which, B), jp.solved_s(which, B))
    print(f"recipe S rig {which}: float32 replay vs double, worst of {B}: {d.max():.2e}; objective after / before, worst: {ratio.max():.2e}")
    assert d.max() <= 1e-5, d
    assert ratio.max() <= 1e-2, ratio


def test_joint_block_marshalling():
    K, B = 3, 2
    a, b = np.array([1, 2, 3], np.int32), np.array([3, 0, 3], np.int32)
    rng = np.random.default_rng(0)
    oa, ob = rng.normal(size=(B, K, 3)).astype(np.float32), rng.normal(size=(B, K, 3)).astype(np.float32)
    w, d = rng.uniform(0.5, 1.5, (B, K)).astype(np.float32), rng.uniform(0.5, 1.5, (B, K)).astype(np.float32)
    blk = _abi.JointBlock(_abi.MMX_JC_JOINT_TO_JOINT_DISTANCE, a, w, None, local_point=oa, local_dir=ob, plane_d=d, parent_b=b)
    assert blk.count == K and blk.rows == K
    assert list(blk.parent) == [1, 2, 3] and list(blk.parent_b) == [3, 0, 3]
    assert list(blk.parent_array()) == [1, 2, 3, 3, 0, 3]
    keep = []
    s = blk.struct(keep, batch=B)
    assert s.type == 10 and s.count == K and not s.global_ and s.local_point and s.local_dir and s.plane_d and s.weight and not s.projection
    got = np.ctypeslib.as_array(C.cast(s.parent, C.POINTER(C.c_int32)), shape=(2 * K,))
    assert list(got) == [1, 2, 3, 3, 0, 3]  # joints A, then joints B
    one = blk.instance(1)
    assert one.type == blk.type and one.count == K and list(one.parent_b) == [3, 0, 3] and one.global_ is None
    assert np.array_equal(one.local_dir, ob[1]) and np.array_equal(one.local_point, oa[1]) and np.array_equal(one.plane_d, d[1])
    assert np.array_equal(one.weight, w[1])
    # the second parent list belongs to this type, and to it alone
    with pytest.raises(ValueError):
        _abi.JointBlock(_abi.MMX_JC_JOINT_TO_JOINT_DISTANCE, a, w, None, local_point=oa, local_dir=ob, plane_d=d)
    with pytest.raises(ValueError):
        _abi.JointBlock(_abi.MMX_JC_DISTANCE, a, w, oa, local_point=oa, plane_d=d, parent_b=b)
    with pytest.raises(ValueError):
        _abi.JointBlock(_abi.MMX_JC_JOINT_TO_JOINT_DISTANCE, a, w, None, local_point=oa, local_dir=ob, plane_d=d, parent_b=b[:2])
    # every other type keeps its [count] parent array
    plain = _abi.JointBlock(_abi.MMX_JC_DISTANCE, a, w, oa, local_point=oa, plane_d=d)
    assert plain.parent_b is None and list(plain.parent_array()) == [1, 2, 3]


def test_solver2_class_lowers_to_one_pair_block():
    rig = make_test_character(4)
    ch = solver2.Character(rig)
    f = solver2.JointToJointDistanceErrorFunction(ch, weight=0.5)
    f.add_constraint(3, [0.0, 0.1, 0.0], 1, [0.2, 0.0, 0.0], 0.75, weight=1.5, name="pinch")
    f.add_constraints([2, 3], np.zeros((2, 3)), [0, 3], np.array([[0.0, 0.0, 0.1], [0.0, 0.0, 0.2]]), np.array([0.3, 0.4]))
    blk = f.block(2)
    assert blk.type == _abi.MMX_JC_JOINT_TO_JOINT_DISTANCE and blk.function_weight == 0.5 and blk.loss == (2.0, 1.0)
    assert blk.count == 3 and blk.rows == 3 and blk.global_ is None
    assert list(blk.parent) == [3, 2, 3] and list(blk.parent_b) == [1, 0, 3]
    assert blk.local_point.shape == (2, 3, 3) and np.allclose(blk.local_point[1, 0], [0.0, 0.1, 0.0])
    assert np.allclose(blk.local_dir[0, 0], [0.2, 0.0, 0.0]) and np.allclose(blk.local_dir[1, 2], [0.0, 0.0, 0.2])
    assert np.allclose(blk.plane_d, [[0.75, 0.3, 0.4]] * 2) and np.allclose(blk.weight, [[1.5, 1.0, 1.0]] * 2)
    with pytest.raises(RuntimeError):
        f.add_constraint(0, np.zeros(3), 4, np.zeros(3), 1.0)  # second joint out of range
    with pytest.raises(RuntimeError):
        f.add_constraint(7, np.zeros(3), 0, np.zeros(3), 1.0)
    assert len(f.constraints) == 3
    f.clear_constraints()
    f.add_constraint(1, np.zeros(3), 2, np.zeros(3), 1.0)
    assert list(f.block(1).parent_b) == [2]
