"""The matrix-free gradient through the C++ shell (BatchedSkeletonSolverFunction::getGradient and
SkeletonSolverFunction::getGradient, include/momentum_amd/momentum_amd.hpp): the program compiles and links everywhere, and on
the GPU the gradient equals 2 J^T r of the same function's getJacobian within the bound the program derives, the error its
error, and the single-instance function the batch's row bit for bit (tests/cpp/test_shell_gradient.cpp)."""
import os
import subprocess

import pytest

from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_shell_gradient.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_shell_gradient")


def _compile():
    mbuild.build()
    libdir = os.path.join(ROOT, "momentum_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lmmx_hip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]  # fmt: skip
    subprocess.check_call(cmd)


def test_cpp_shell_gradient_program_compiles_and_links():
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_shell_gradient_program_runs_on_gpu():
    _compile()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
