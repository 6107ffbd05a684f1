"""The rig-level tables of mmx_eval_skeleton_state_backward (buildStateBackwardTables in momentum_amd/csrc/mmx_host_tables.cpp)
and its LDS budget rule (stateBackwardRefusal in mmx_solve_plan.cpp) on the CPU, under the address and undefined-behaviour
sanitizers: the all-parameter source lists equal a brute-force transpose of the CSR transform, entry for entry and in row order
(tests/cpp/test_state_backward_tables.cpp: a stand-alone program that links the two host files and nothing else)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_state_backward_tables.cpp")
HOST = [os.path.join(ROOT, "momentum_amd", "csrc", f) for f in ("mmx_host_tables.cpp", "mmx_solve_plan.cpp")]


def test_state_backward_tables_match_their_restatements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_state_backward_tables")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, *HOST, "-o", exe]  # fmt: skip
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
