"""The closest-point-on-mesh query through the C++ shell (DeviceMesh::closestPoints / findClosestPointsOnMesh,
include/momentum_amd/momentum_amd.hpp): the program compiles and links everywhere, and on the GPU its results agree with a
brute force written in the program within the bounds it states (tests/cpp/test_shell_closest_points_on_mesh.cpp)."""
import os
import subprocess

import pytest

from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_shell_closest_points_on_mesh.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_shell_closest_points_on_mesh")


def _compile():
    mbuild.build()
    libdir = os.path.join(ROOT, "momentum_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lmmx_hip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]  # fmt: skip
    subprocess.check_call(cmd)


def test_cpp_shell_closest_points_on_mesh_program_compiles_and_links():
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_shell_closest_points_on_mesh_program_runs_on_gpu():
    _compile()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
