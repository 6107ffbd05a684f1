"""The constraint intake of momentum_amd/csrc/mmx_constraint_intake.{hpp,cpp} (every check of mmx_problem_set_constraints and
mmx_problem_set_instance_parents, the integers they derive and the comparison with the previous state that decides whether the
tables are rebuilt) against a transcription of the code it replaced, over generated requests, on the CPU and under the address
and undefined-behaviour sanitizers (tests/cpp/test_constraint_intake.cpp: a stand-alone program that links the host unit and
mmx_host_tables.cpp, nothing else)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_constraint_intake.cpp")
HOST = [os.path.join(ROOT, "momentum_amd", "csrc", f) for f in ("mmx_constraint_intake.cpp", "mmx_host_tables.cpp")]


def test_constraint_intake_matches_the_transcribed_setters_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_constraint_intake")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, *HOST, "-o", exe]  # fmt: skip
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
