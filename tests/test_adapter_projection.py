"""integration/tensor_ik_mmx_adapter.cpp with the Projection and Distance slots of solve_ik: it compiles against the stub of
the reference types, and on the GPU a projection batch through solveBatch is bit-identical to the same problem sent through
momentum_amd.capi (tests/cpp/adapter_projection.cpp makes the batch up and writes it with its answer)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from momentum_amd import _abi, make_test_character
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "adapter_projection.cpp")


def _compile(out_dir):
    mbuild.build()
    libdir = os.path.join(ROOT, "momentum_amd")
    idir = os.path.join(ROOT, "integration")
    exe = os.path.join(out_dir, "adapter_projection")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", idir,
                           os.path.join(idir, "tensor_ik_mmx_adapter.cpp"), SRC, "-L", libdir, "-lmmx_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])  # fmt: skip
    return exe


def test_adapter_with_projection_slots_compiles():
    with tempfile.TemporaryDirectory() as td:
        assert os.path.exists(_compile(td))


@pytest.mark.gpu
def test_adapter_projection_batch_is_bit_identical_to_capi():
    import torch

    from momentum_amd import capi

    B, Kp, Kq, Kd, P = 8, 1, 3, 1, 10
    with tempfile.TemporaryDirectory() as td:
        exe = _compile(td)
        out = os.path.join(td, "out.bin")
        run = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
        data = np.fromfile(out, np.float32)
    sizes = [B * Kp * 3, B * Kq * 3, B * Kq * 12, B * Kq * 2, B * Kd * 3, B * Kd, B * P]
    assert data.size == sum(sizes)
    pos_tgt, proj_off, proj, proj_tgt, dist_origin, dist_tgt, theta_adapter = np.split(data, np.cumsum(sizes)[:-1])
    uvw = np.zeros((B, Kq, 3), np.float32)
    uvw[..., :2] = proj_tgt.reshape(B, Kq, 2)
    blocks = [
        _abi.JointBlock(_abi.MMX_JC_PROJECTION, [1, 2, 2], np.ones((B, Kq), np.float32), uvw, local_point=proj_off.reshape(B, Kq, 3),
                        projection=proj.reshape(B, Kq, 12), near_clip=0.5),
        _abi.JointBlock(_abi.MMX_JC_DISTANCE, [2], np.ones((B, Kd), np.float32), dist_origin.reshape(B, Kd, 3),
                        local_point=np.zeros((B, Kd, 3), np.float32), plane_d=dist_tgt.reshape(B, Kd)),
    ]  # fmt: skip
    pb = capi.Problem(capi.RigHandle(make_test_character(3), 0), B, [2], [])
    pb.set_constraints(np.zeros((B, Kp, 3), np.float32), pos_tgt.reshape(B, Kp, 3), np.ones((B, Kp), np.float32),
                       np.zeros((B, 0, 4), np.float32), np.zeros((B, 0, 4), np.float32), np.zeros((B, 0), np.float32), joint_blocks=blocks)  # fmt: skip
    opt = _abi.GnOptions.make(min_iterations=6, max_iterations=6, threshold=1.0, regularization=0.05)
    th = torch.zeros((B, P), dtype=torch.float32, device=pb.device)
    pb.solve(th, opt)
    got = th.cpu().numpy()
    assert np.any(got != 0)
    assert np.array_equal(got, theta_adapter.reshape(B, P))
