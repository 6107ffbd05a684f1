"""mmx_eval_gradient's scope decision (gradientRefusal in momentum_amd/csrc/mmx_solve_plan.cpp) on the CPU, under the address and
undefined-behaviour sanitizers: every refusal alone and in pairs, the first in the documented order reported, the all-clear
case accepted (tests/cpp/test_gradient_plan.cpp: a stand-alone program that links the one host file and nothing else)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_gradient_plan.cpp")
HOST = os.path.join(ROOT, "momentum_amd", "csrc", "mmx_solve_plan.cpp")


def test_gradient_refusals_in_their_documented_order_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_gradient_plan")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, HOST, "-o", exe]  # fmt: skip
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
