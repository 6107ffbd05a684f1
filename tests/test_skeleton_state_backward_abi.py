"""mmx_eval_skeleton_state_backward / _host at the C-ABI boundary (no GPU needed): include/mmx.h declares them with their
parameter lists, the ctypes binding lists them with argument types, and the built library exports them -- a library that
predates the functions lacks the symbols, which is the feature probe (MMX_ABI_VERSION does not move)."""
import ctypes as C
import os
import re

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "mmx_eval_skeleton_state_backward": ["mmx_problem* problem", "const float* theta_dev", "const float* state_grad_dev", "float* theta_grad_dev", "void* stream"],
    "mmx_eval_skeleton_state_backward_host": ["mmx_problem* problem", "const float* theta_host", "const float* state_grad_host", "float* theta_grad_host"],
}


def test_declared_in_header_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmx.h")).read(), flags=re.S)
    for name, want in PARAMS.items():
        m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"include/mmx.h does not declare {name}"
        assert name in capi.SYMBOLS
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == want, params
    assert _abi.MMX_ABI_VERSION == 12
    assert re.search(r"#define\s+MMX_ABI_VERSION\s+12\b", src)


def test_library_exports_them():
    mbuild.build()
    L = capi.lib()
    for name, want in PARAMS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), name
        assert all(a is C.c_void_p for a in fn.argtypes), (name, fn.argtypes)
    assert L.mmx_abi_version() == _abi.MMX_ABI_VERSION == 12
    assert hasattr(capi.Problem, "skeleton_state_backward")
    from momentum_amd import autograd

    assert callable(autograd.skeleton_state)


def test_backward_kernel_is_a_translation_unit_of_its_own_without_scratch():
    """mmx_state_backward.hip is built with the default pipeline like mmx_gradient.hip, holds one kernel, and that kernel uses
    no scratch memory and spills no vector register."""
    import subprocess
    import tempfile

    assert "mmx_state_backward.hip" in mbuild.SOURCES and mbuild._extra_flags("mmx_state_backward.hip", None) == []
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_state_backward.hip"),
               "-o", os.path.join(td, "g.o"), "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    kernels = re.split(r"remark: Function Name: ", r.stderr.decode(errors="replace"))[1:]
    assert len(kernels) == 1, kernels
    k = kernels[0]
    get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
    fig = {key: get(key) for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill")}
    print(k.split()[0], fig)
    assert "skeletonStateBackwardKernel" in k.split()[0]
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, fig
