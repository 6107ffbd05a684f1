"""The solver's step and stopping rules of momentum_amd/csrc/mmx_solver_rules.hpp (convergence, LM schedule, both backtracking
rules, the trust region's decisions, the acceptance of a refinement step, the precision estimate, the status word) against a
transcription of the expressions the solve kernels spelled out before the header existed, bit for bit, on the CPU and under
the address and undefined-behaviour sanitizers (tests/cpp/test_solver_rules.cpp: a stand-alone program, the header alone) --
and a mutation pass over the header: every comparison flipped and every constant changed, one at a time, must make that
program fail."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_solver_rules.cpp")
HEADER = os.path.join(ROOT, "momentum_amd", "csrc", "mmx_solver_rules.hpp")

FLIP = {">=": "<", "<=": ">", ">": "<=", "<": ">=", "==": "!="}
# Mutants the program cannot tell from the header, each with its reason (keyed by line text and column): none is tolerated
# without one.
SURVIVORS = {}


def test_solver_rules_match_the_transcribed_sites_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_solver_rules")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout


def _mutants(text):
    """(description, mutated text) for every comparison and every constant in the code of the header's functions and constants."""
    out = []
    pos = 0
    for line in text.splitlines(keepends=True):
        code = line.split("//")[0]
        body = code.startswith("  ") or code.startswith("constexpr ")  # a function's statements, or a constant of the rules
        if body and not code.lstrip().startswith(("#", "template", "static_assert")):
            for m in re.finditer(r"(?<![<>=!\-])(>=|<=|==|>|<)(?![<>=])", code):
                out.append((f"{line.strip()[:70]} @{m.start()}: {m.group(1)} -> {FLIP[m.group(1)]}", pos + m.start(), m.end() - m.start(), FLIP[m.group(1)]))
            for m in re.finditer(r"(?<![\w.])(\d+\.?\d*(?:e-?\d+)?)(f?)(?![\w.])", code):
                v = float(m.group(1))
                new = ("1" if v == 0 else repr(v * 2) if ("." in m.group(1) or "e" in m.group(1)) else str(int(v) * 2)) + m.group(2)
                out.append((f"{line.strip()[:70]} @{m.start()}: {m.group(0)} -> {new}", pos + m.start(), m.end() - m.start(), new))
            for m in re.finditer(r"\bFLT_(EPSILON|MIN)\b", code):
                out.append((f"{line.strip()[:70]} @{m.start()}: {m.group(0)} doubled", pos + m.start(), m.end() - m.start(), f"(2 * {m.group(0)})"))
        pos += len(line)
    return [(d, text[:p] + new + text[p + n :]) for d, p, n, new in out]


def test_every_mutant_of_the_header_is_caught(tmp_path):
    with open(HEADER) as f:
        text = f.read().replace('"../../include/mmx.h"', '"' + os.path.join(ROOT, "include", "mmx.h") + '"')
    mutants = _mutants(text)
    assert len(mutants) >= 40, len(mutants)

    def caught(job):
        i, (_, mutated) = job
        hdr, exe = str(tmp_path / f"m{i}.hpp"), str(tmp_path / f"m{i}")
        with open(hdr, "w") as f:
            f.write(mutated)
        cc = subprocess.run(["g++", "-std=c++17", "-O0", f'-DMMX_RULES_HEADER="{hdr}"', SRC, "-o", exe], capture_output=True, text=True)
        if cc.returncode != 0:  # (a constant the program holds with a static_assert of its own, named by its message)
            return "rules constant differs from the sites" in cc.stderr
        return subprocess.run([exe], capture_output=True, text=True, timeout=120).returncode != 0

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        verdicts = list(ex.map(caught, enumerate(mutants)))
    survivors = [d for (d, _), c in zip(mutants, verdicts) if not c]
    print(f"{sum(verdicts)} of {len(mutants)} mutants caught; survivors: {survivors}")
    unexplained = [d for d in survivors if not any(k in d for k in SURVIVORS)]
    assert not unexplained, unexplained
