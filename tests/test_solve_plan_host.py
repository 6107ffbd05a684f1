"""The solve planner of momentum_amd/csrc/mmx_solve_plan.{hpp,cpp} (which kernels a solve call runs, or the refusal it gets)
against a transcription of the dispatch it replaced, over the full product of the facts the decision reads, on the CPU and under
the address and undefined-behaviour sanitizers (tests/cpp/test_solve_plan.cpp: a stand-alone program that links the one host
file and nothing else)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_solve_plan.cpp")
HOST = os.path.join(ROOT, "momentum_amd", "csrc", "mmx_solve_plan.cpp")


def test_solve_plan_matches_the_transcribed_dispatch_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_solve_plan")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, HOST, "-o", exe]  # fmt: skip
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
