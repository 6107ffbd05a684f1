"""CPU checks of MMX_ROUTE_WAVE's additions: the header's constants against the ctypes mirror (ABI version unchanged), the build
recipe (a new translation unit, the existing ones' flags as they were), and the kernel's register report (no scratch, no spills)."""
import os
import re
import subprocess
import tempfile

from momentum_amd import _abi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_constants_match_mirror():
    prog = r"""
    #include <stdio.h>
    #include "mmx.h"
    int main(void) {
      printf("%d %d %d %d %d\n", MMX_ROUTE_WAVE, MMX_WAVE_MAX_JOINTS, MMX_WAVE_MAX_SOLVED, MMX_WAVE_MAX_UNITS, MMX_ABI_VERSION);
      return 0;
    }"""
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out == [_abi.ROUTES["wave"], _abi.WAVE_MAX_JOINTS, _abi.WAVE_MAX_SOLVED, _abi.WAVE_MAX_UNITS, 12]
    assert out[:3] == [4, 64, 32]
    assert _abi.MMX_ABI_VERSION == 12
    assert sorted(_abi.ROUTES.values()) == [0, 1, 2, 3, 4]
    # the position + orientation blocks on all 24 joints of the chain (24 + 3 x 24 units) are inside the cap
    assert _abi.WAVE_MAX_UNITS >= 24 + 3 * 24


def test_build_recipe_has_the_new_unit_and_keeps_the_old_flags():
    assert "mmx_wave.hip" in mbuild.SOURCES
    assert os.path.exists(os.path.join(mbuild.CSRC, "mmx_wave.hip"))
    solve = ["-mllvm", "-disable-machine-licm", "-mllvm", "-disable-lsr"]
    assert mbuild._extra_flags("mmx_fused.hip", 0) == solve and mbuild._extra_flags("mmx_fused.hip", 4) == []
    assert mbuild._extra_flags("mmx_f64.hip", None) == solve
    for src in ("mmx_kernels.hip", "mmx_capi.hip", "mmx_comm.hip", "mmx_host_tables.cpp"):
        assert mbuild._extra_flags(src, None) == []
    assert mbuild._extra_flags("mmx_wave.hip", None) == []  # the default pipeline
    assert mbuild.FUSED_GROUPS == 7


def test_wave_kernels_use_no_scratch_and_spill_nothing():
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_wave.hip"),
               "-o", os.path.join(td, "w.o"), "-Rpass-analysis=kernel-resource-usage"] + mbuild._extra_flags("mmx_wave.hip", None)  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    text = r.stderr.decode(errors="replace")
    kernels = re.split(r"remark: Function Name: ", text)[1:]
    assert len(kernels) == 2, text[-2000:]  # the 16- and the 32-column instantiation
    for k in kernels:
        name = k.split()[0]
        get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
        fig = {key: get(key) for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")}
        print(name, fig)
        assert "waveSolveKernel" in name
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["SGPRs Spill"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
