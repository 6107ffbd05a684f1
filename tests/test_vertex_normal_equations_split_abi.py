"""mmx_skin_normal_equations_split at the C-ABI boundary (no GPU needed): include/mmx.h declares the six entry points with
their parameter lists, the ctypes binding lists them with argument types, and the built library exports them -- a library that
predates the functions lacks the symbols, which is the feature probe (MMX_ABI_VERSION does not move).  Refusals that need no
device come back before the first HIP call, and the kernels' translation unit uses no scratch memory and spills no vector
register."""
import ctypes as C
import os
import re

import numpy as np

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "mmx_skin_normal_equations_split": ("int32_t", ["mmx_problem* problem", "mmx_skin* skin", "const mmx_vertex_constraints* constraints",
                                                    "const float* theta_dev", "float* jtj_dev", "float* jtr_dev", "double* err_dev", "int32_t parts",
                                                    "void* workspace_dev", "int64_t workspace_bytes", "void* stream"]),
    "mmx_skin_normal_equations_split_host": ("int32_t", ["mmx_problem* problem", "mmx_skin* skin", "const mmx_vertex_constraints* constraints",
                                                         "const float* theta_host", "float* jtj_host", "float* jtr_host", "double* err_host",
                                                         "int32_t parts"]),
    "mmx_skin_normal_equations_workspace_bytes": ("int64_t", ["int32_t batch", "int32_t num_enabled", "int32_t parts"]),
    "mmx_skin_normal_equations_plan": ("int32_t", ["int32_t batch", "int32_t type", "int32_t count", "int32_t compute_units",
                                                   "int32_t workgroups_per_cu", "int32_t* parts_out"]),
    "mmx_skin_normal_equations_auto_parts": ("int32_t", ["mmx_problem* problem", "mmx_skin* skin", "const mmx_vertex_constraints* constraints",
                                                         "int32_t* parts_out"]),
    "mmx_skin_normal_equations_part_range": ("int32_t", ["int32_t tiles", "int32_t parts", "int32_t part", "int32_t* begin_out", "int32_t* end_out",
                                                         "int32_t* effective_parts_out"]),
}  # fmt: skip


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmx.h")).read(), flags=re.S)


def test_declared_in_header_and_bound():
    src = _header()
    for name, (ret, want) in PARAMS.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), src)
        assert m, f"include/mmx.h does not declare {name}"
        assert name in capi.SYMBOLS
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == want
        types = _abi.SKIN_NORMAL_EQUATIONS_SPLIT_ARGTYPES[name]
        assert len(types) == len(want), name
        for t, p in zip(types, want):
            if p.startswith("int32_t "):
                assert t is C.c_int32, (name, p)
            elif p.startswith("int64_t "):
                assert t is C.c_int64, (name, p)
            elif p.startswith("int32_t* "):
                assert t is _abi.c_int32_p, (name, p)
            elif p.startswith("const mmx_vertex_constraints*"):
                assert t == C.POINTER(_abi.VertexConstraints), (name, p)
            else:
                assert t is C.c_void_p, (name, p)
    assert _abi.MMX_ABI_VERSION == 12
    assert re.search(r"#define\s+MMX_ABI_VERSION\s+12\b", src)
    assert re.search(r"#define\s+MMX_SKIN_NE_MAX_PARTS\s+512\b", src) and _abi.MMX_SKIN_NE_MAX_PARTS == 512


def test_library_exports_them():
    mbuild.build()
    L = capi.lib()
    for name, (_, want) in PARAMS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), name
    assert L.mmx_skin_normal_equations_workspace_bytes.restype is C.c_int64
    assert L.mmx_abi_version() == _abi.MMX_ABI_VERSION == 12
    assert "mmx_skin_normal_equations_plan.cpp" in mbuild.SOURCES and "mmx_skin_normal_equations_plan.hpp" in mbuild.HEADERS
    assert capi.skin_normal_equations_workspace_bytes(1, 128, 2) > 2 * 10 * 4096
    assert capi.skin_normal_equations_plan(16, 20000, plane=False, compute_units=256, workgroups_per_cu=2) == 32
    import inspect

    from momentum_amd import geometry

    for fn in (capi.Problem.vertex_normal_equations, geometry.vertex_normal_equations):
        sig = inspect.signature(fn).parameters
        assert sig["parts"].default == 1 and sig["workspace"].default is None  # the defaults do not change: the unsplit call
    assert callable(capi.Problem.vertex_normal_equations_parts)


def test_refusals_that_need_no_device_come_before_the_first_hip_call():
    """Null handles and an out-of-range `parts` are refused by host code: a status, the function's name in mmx_last_error(), the
    outputs untouched -- on a machine without a GPU as well."""
    mbuild.build()
    L = capi.lib()
    H = np.full((1, 2, 2), -7.25, np.float32)
    g, e = np.full((1, 2), -7.25, np.float32), np.full(1, -7.25, np.float64)
    theta, tgt = np.zeros((1, 4), np.float32), np.zeros((1, 1, 3), np.float32)
    d = _abi.VertexConstraints(_abi.MMX_VC_POSITION, 1, 1, 1.0, None, None, tgt.ctypes.data, None, None, None)
    p = lambda a: C.c_void_p(a.ctypes.data)
    out = C.c_int32(-5)
    calls = {
        "mmx_skin_normal_equations_split": lambda: L.mmx_skin_normal_equations_split(None, None, C.byref(d), p(theta), p(H), p(g), p(e), 2, None, 0, None),
        "mmx_skin_normal_equations_split_host": lambda: L.mmx_skin_normal_equations_split_host(None, None, C.byref(d), p(theta), p(H), p(g), p(e), 2),
        "mmx_skin_normal_equations_auto_parts": lambda: L.mmx_skin_normal_equations_auto_parts(None, None, C.byref(d), C.byref(out)),
    }  # fmt: skip
    for name, call in calls.items():
        rc = call()
        assert rc != 0 and L.mmx_last_error().decode() != "", name
        assert (H == -7.25).all() and (g == -7.25).all() and (e == -7.25).all() and out.value == -5, name
    assert L.mmx_skin_normal_equations_split_host(None, None, C.byref(d), p(theta), p(H), p(g), p(e), -1) != 0
    assert (H == -7.25).all() and (g == -7.25).all() and (e == -7.25).all()
    assert L.mmx_skin_normal_equations_workspace_bytes(1, 5, 513) == -1 and L.mmx_skin_normal_equations_workspace_bytes(1, 5, 1) == 0
    assert L.mmx_skin_normal_equations_plan(0, 0, 5, 256, 2, C.byref(out)) == 1 and out.value == -5


def test_kernels_compile_for_gfx950_without_scratch():
    """mmx_skin_normal_equations.hip is built with the default pipeline; its three kernels -- the unsplit and the split
    instantiation of skinNormalEquationsKernel and skinNormalEquationsReduceKernel -- use no scratch memory and spill no vector
    register, and the two instantiations keep two waves per SIMD (two workgroups per compute unit): the figures printed here are
    the ones DESIGN.md quotes."""
    import subprocess
    import tempfile

    assert mbuild._extra_flags("mmx_skin_normal_equations.hip", None) == []
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_skin_normal_equations.hip"),
               "-o", os.path.join(td, "c.o"), "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    kernels = re.split(r"remark: (?:\S+: )?Function Name: ", r.stderr.decode(errors="replace"))[1:]
    names = sorted(k.split()[0] for k in kernels)
    assert len(kernels) == 3, names
    assert sum("skinNormalEquationsKernel" in nm for nm in names) == 2 and sum("skinNormalEquationsReduceKernel" in nm for nm in names) == 1, names
    for k in kernels:
        get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
        fig = {key: get(key) for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill")}
        print(k.split()[0], fig)
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (k.split()[0], fig)
        assert fig["Occupancy [waves/SIMD]"] >= 2, (k.split()[0], fig)
