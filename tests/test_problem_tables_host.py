"""The problem-table builders of momentum_amd/csrc/mmx_host_tables.{hpp,cpp} (what uploadProblemTables / uploadSolveView of
mmx_capi.hip copy to the device) against brute-force restatements, on the CPU and under the address and undefined-behaviour
sanitizers (tests/cpp/test_problem_tables.cpp: a stand-alone program that links the one host file and nothing else)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_problem_tables.cpp")
HOST = os.path.join(ROOT, "momentum_amd", "csrc", "mmx_host_tables.cpp")


def test_problem_tables_match_their_restatements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_problem_tables")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, HOST, "-o", exe]  # fmt: skip
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
