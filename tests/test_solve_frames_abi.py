"""mmx_solve_frames / mmx_solve_frames_host at the C-ABI boundary (no GPU needed): include/mmx.h declares them, the ctypes
binding lists them with argument types, and the built library exports them -- a library that predates the functions lacks the
symbols, which is the feature probe (MMX_ABI_VERSION does not move)."""
import ctypes as C
import os
import re

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_solve_frames", "mmx_solve_frames_host")


def test_declared_in_header_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmx.h")).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"include/mmx.h does not declare {name}"
        assert name in capi.SYMBOLS
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[2] == "int32_t num_frames", params
        assert len(params) == (10 if name == "mmx_solve_frames" else 7), params
    assert _abi.MMX_ABI_VERSION == 12


def test_library_exports_them():
    mbuild.build()
    L = capi.lib()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.argtypes[2] is C.c_int32, name
    assert len(L.mmx_solve_frames.argtypes) == 10 and len(L.mmx_solve_frames_host.argtypes) == 7
    assert L.mmx_abi_version() == _abi.MMX_ABI_VERSION
    assert hasattr(capi.Problem, "solve_frames")


def test_frames_kernels_use_no_scratch_and_spill_nothing():
    """The two frame-sequence instantiations (their own translation unit, mmx_wave_frames.hip) keep the register notes of the
    kernel they share with mmx_solve: no scratch, no spilled register, the occupancy of the plain instantiations."""
    import subprocess
    import tempfile

    assert "mmx_wave_frames.hip" in mbuild.SOURCES and mbuild._extra_flags("mmx_wave_frames.hip", None) == []
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_wave_frames.hip"),
               "-o", os.path.join(td, "w.o"), "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    kernels = re.split(r"remark: Function Name: ", r.stderr.decode(errors="replace"))[1:]
    assert len(kernels) == 2, kernels  # the 16- and the 32-column instantiation, kFrames = true
    for k in kernels:
        name = k.split()[0]
        get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
        fig = {key: get(key) for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")}
        print(name, fig)
        assert "waveSolveKernel" in name and "Lb1E" in name, name
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["SGPRs Spill"] == 0 and fig["VGPRs Spill"] == 0, (name, fig)
        assert fig["Occupancy [waves/SIMD]"] == 3, (name, fig)
