"""The split of mmx_skin_normal_equations_split (momentum_amd/csrc/mmx_skin_normal_equations_plan.cpp) on the CPU, under the
address and undefined-behaviour sanitizers: the part ranges, the workspace's offsets (no two regions overlap, the last ends
within the reported size), the plan, and every refusal of the split with its status, a message that names the condition and
the order (tests/cpp/test_skin_normal_equations_plan.cpp: a stand-alone program that links the host file and nothing else)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_skin_normal_equations_plan.cpp")
HOST = [os.path.join(ROOT, "momentum_amd", "csrc", "mmx_skin_normal_equations_plan.cpp")]


def test_skin_normal_equations_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_skin_normal_equations_plan")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, *HOST, "-o", exe]  # fmt: skip
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
