"""CPU checks of the projection / distance joint blocks (include/mmx.h ABI 12): the grown block struct against its ctypes
mirror, the constants, the double reference's analytic rows against central differences, and the solver2 classes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from momentum_amd import _abi, humanoid72_landmark_joints, make_humanoid72, make_test_character, solver2
from tests import projection_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grown_block_layout_matches_header():
    prog = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "mmx.h"
    int main(void) {
      printf("%zu %zu %zu %zu %d\n", sizeof(mmx_joint_constraint_block), offsetof(mmx_joint_constraint_block, loss_c),
             offsetof(mmx_joint_constraint_block, projection), offsetof(mmx_joint_constraint_block, near_clip), MMX_ABI_VERSION);
      printf("%d %d %d\n", MMX_JC_PROJECTION, MMX_JC_DISTANCE, MMX_MAX_JOINT_BLOCKS);
      return 0;
    }"""
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    B = _abi.JointConstraintBlock
    assert got[:5] == [C.sizeof(B), B.loss_c.offset, B.projection.offset, B.near_clip.offset, _abi.MMX_ABI_VERSION]
    assert B.projection.offset > B.loss_c.offset and B.near_clip.offset > B.projection.offset  # grown at its end
    assert got[5:] == [_abi.MMX_JC_PROJECTION, _abi.MMX_JC_DISTANCE, _abi.MMX_MAX_JOINT_BLOCKS]


def test_constants_and_func_dims():
    assert _abi.MMX_ABI_VERSION == 12
    assert (_abi.MMX_JC_PROJECTION, _abi.MMX_JC_DISTANCE) == (8, 9)
    assert _abi.jc_func_dim(_abi.MMX_JC_PROJECTION) == 2
    assert _abi.jc_func_dim(_abi.MMX_JC_DISTANCE) == 1
    blk = _abi.JointBlock(_abi.MMX_JC_PROJECTION, [1, 2, 3], np.ones(3), np.zeros((3, 3)), local_point=np.zeros((3, 3)), projection=np.zeros((3, 12)))
    assert blk.rows == 6 and blk.near_clip == 1.0
    keep = []
    s = blk.struct(keep)
    assert s.type == _abi.MMX_JC_PROJECTION and s.projection and s.near_clip == 1.0


def _fd_check(rig, base, blocks, theta, h=1e-6):
    J, r, e = pr.full_rows(rig, base, blocks, theta)
    assert abs(r @ r - e) <= 1e-9 * max(1.0, e)
    for p in range(rig.num_params):
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        fd = (pr.full_rows(rig, base, blocks, tp)[1] - pr.full_rows(rig, base, blocks, tm)[1]) / (2 * h)
        assert np.abs(fd - J[:, p]).max() <= 1e-5 * max(1.0, np.abs(J[:, p]).max()), (p, np.abs(fd - J[:, p]).max())
    return J, r


def test_reference_rows_match_central_differences_on_the_humanoid():
    rig = make_humanoid72(unit=0.01)
    lm = humanoid72_landmark_joints(rig)
    B = 3
    base, blocks, th0, _ = pr.keypoint_problem(rig, B, 21, lm[:4], lm, n_cams=2, dist_parents=lm[4:8], behind=True)
    rng = np.random.default_rng(3)
    for b in range(B):
        inst = [k.instance(b) for k in blocks]
        inst[0].weight = rng.uniform(0.5, 2.0, inst[0].count).astype(np.float32)
        inst[0].local_point = rng.uniform(-0.05, 0.05, (inst[0].count, 3)).astype(np.float32)
        J, r = _fd_check(rig, base.instance(b), inst, th0[b].astype(np.float64))
        # the constraint behind the camera: its two rows are exactly zero
        first = 3 * base.Kp + 2 * (inst[0].count - 1)
        assert np.all(J[first:first + 2] == 0) and np.all(r[first:first + 2] == 0)


def test_near_clip_skips_only_constraints_in_front_of_the_plane():
    rig = make_test_character(4)
    x, _ = pr.world_points(rig, [3], np.zeros((1, 3)), np.zeros(rig.num_params))
    cam = pr.look_at_camera(x[0] + np.array([0.0, 0.0, -3.0]), x[0], 2.0)  # depth 3
    for near, clipped in ((1.0, False), (2.9, False), (3.1, True)):
        blk = _abi.JointBlock(_abi.MMX_JC_PROJECTION, [3], np.ones(1), np.array([[0.1, 0.2, 0.0]]), local_point=np.zeros((1, 3)),
                              projection=cam.reshape(1, 12), near_clip=near)  # fmt: skip
        f, d, c = pr.block_eval(blk, x)
        assert bool(c[0]) == clipped
        assert np.allclose(f[0], [0.0, 0.0] if clipped else [-0.1, -0.2], atol=1e-6)


def test_solver2_classes_build_the_expected_blocks():
    rig = make_test_character(4)
    ch = solver2.Character(rig)
    cam = pr.look_at_camera([0.0, 1.0, -4.0], [0.0, 1.0, 0.0], 3.0)
    pf = solver2.ProjectionErrorFunction(ch, near_clip=0.5, weight=2.0)
    pf.add_constraint(cam, 3, [0.1, 0.2], offset=[0.0, 0.5, 0.0], weight=1.5)
    pf.add_constraint(cam, 2, [0.3, 0.4])
    blk = pf.block(2)
    assert blk.type == _abi.MMX_JC_PROJECTION and blk.near_clip == 0.5 and blk.function_weight == 2.0 and blk.loss == (2.0, 1.0)
    assert list(blk.parent) == [3, 2] and blk.rows == 4
    assert blk.projection.shape == (2, 2, 12) and np.allclose(blk.projection[1, 0], cam.reshape(-1))
    assert np.allclose(blk.global_[0, 0], [0.1, 0.2, 0.0]) and np.allclose(blk.local_point[1, 0], [0.0, 0.5, 0.0])
    assert np.allclose(blk.weight, [[1.5, 1.0], [1.5, 1.0]])
    df = solver2.DistanceErrorFunction(ch, weight=0.5)
    df.add_constraints(np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), np.array([2.0, 3.0]), [1, 3])
    blk = df.block(1)
    assert blk.type == _abi.MMX_JC_DISTANCE and blk.function_weight == 0.5 and blk.rows == 2
    assert np.allclose(blk.plane_d, [[2.0, 3.0]]) and np.allclose(blk.global_[0, 1], [1.0, 0.0, 0.0]) and np.allclose(blk.local_point, 0.0)
