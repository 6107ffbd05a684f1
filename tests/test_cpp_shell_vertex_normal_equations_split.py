"""The split form of the vertex constraints' Gauss-Newton terms through the C++ shell (the `parts` overloads of
DeviceSkin::normalEquations, include/momentum_amd/momentum_amd.hpp): the program compiles and links everywhere, and on the GPU
parts = 1 gives the bits of the unsplit form, parts beyond the tiles those of parts = tiles, and parts = 3 meets parts = 1
within the bounds the program states (tests/cpp/test_shell_vertex_normal_equations_split.cpp)."""
import os
import subprocess

import pytest

from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_shell_vertex_normal_equations_split.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_shell_vertex_normal_equations_split")


def _compile():
    mbuild.build()
    libdir = os.path.join(ROOT, "momentum_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lmmx_hip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]  # fmt: skip
    subprocess.check_call(cmd)


def test_cpp_shell_vertex_normal_equations_split_program_compiles_and_links():
    _compile()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_shell_vertex_normal_equations_split_program_runs_on_gpu():
    _compile()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
