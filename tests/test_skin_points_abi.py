"""Linear-blend skinning at the C-ABI boundary (no GPU needed): include/mmx.h declares the entry points with their parameter
lists, the ctypes binding lists them with argument types, and the built library exports them -- a library that predates the
functions lacks the symbols, which is the feature probe (MMX_ABI_VERSION does not move)."""
import ctypes as C
import os
import re

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "mmx_skin_create": ("int32_t", ["mmx_rig* rig", "const mmx_skin_desc* desc", "mmx_skin** out"]),
    "mmx_skin_destroy": ("void", ["mmx_skin* skin"]),
    "mmx_skin_num_vertices": ("int32_t", ["const mmx_skin* skin"]),
    "mmx_skin_points": ("int32_t", ["mmx_skin* skin", "int32_t batch", "const float* state_dev", "const float* rest_dev", "float* out_dev", "void* stream"]),
    "mmx_skin_points_backward": ("int32_t", ["mmx_skin* skin", "int32_t batch", "const float* state_dev", "const float* rest_dev", "const float* out_grad_dev",
                                             "float* state_grad_dev", "float* rest_grad_dev", "void* stream"]),
    "mmx_skin_points_host": ("int32_t", ["mmx_skin* skin", "int32_t batch", "const float* state_host", "const float* rest_host", "float* out_host"]),
    "mmx_skin_points_backward_host": ("int32_t", ["mmx_skin* skin", "int32_t batch", "const float* state_host", "const float* rest_host",
                                                  "const float* out_grad_host", "float* state_grad_host", "float* rest_grad_host"]),
    "mmx_host_skin_tables": ("int32_t", ["int32_t num_joints", "const mmx_skin_desc* desc", "int32_t* joint_start", "int32_t* entry_vertex",
                                         "int32_t* entry_slot", "int32_t* num_entries"]),
}  # fmt: skip
DESC_FIELDS = ["int32_t num_vertices", "int32_t max_influences", "const int32_t* joint", "const float* weight", "const float* inverse_bind",
               "const float* rest_positions"]  # fmt: skip


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmx.h")).read(), flags=re.S)


def test_declared_in_header_and_bound():
    src = _header()
    for name, (ret, want) in PARAMS.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), src)
        assert m, f"include/mmx.h does not declare {name}"
        assert name in capi.SYMBOLS
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == want, params
    m = re.search(r"typedef\s+struct\s+mmx_skin_desc\s*\{([^}]*)\}\s*mmx_skin_desc\s*;", src)
    assert m, "include/mmx.h does not define mmx_skin_desc"
    assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == DESC_FIELDS
    assert [f for f, _ in _abi.SkinDesc._fields_] == [f.split()[-1].lstrip("*") for f in DESC_FIELDS]
    assert re.search(r"#define\s+MMX_MAX_SKIN_INFLUENCES\s+8\b", src) and _abi.MMX_MAX_SKIN_INFLUENCES == 8
    assert _abi.MMX_ABI_VERSION == 12
    assert re.search(r"#define\s+MMX_ABI_VERSION\s+12\b", src)


def test_library_exports_them():
    mbuild.build()
    L = capi.lib()
    for name, (_, want) in PARAMS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), name
    assert all(a is C.c_void_p for a in L.mmx_skin_points_backward.argtypes[2:]), L.mmx_skin_points_backward.argtypes
    assert L.mmx_abi_version() == _abi.MMX_ABI_VERSION == 12
    assert L.mmx_skin_num_vertices(None) == 0
    for method in ("skin_points", "skin_points_backward"):
        assert hasattr(capi.Skin, method)
    from momentum_amd import autograd, rigs

    assert callable(autograd.skin_points) and callable(rigs.make_test_skin)


def test_skinning_kernels_are_a_translation_unit_of_their_own_without_scratch():
    """mmx_skinning.hip is built with the default pipeline like mmx_gradient.hip; every kernel in it (the forward, its
    rest-gradient instantiation, the backward) uses no scratch memory and spills no vector register."""
    import subprocess
    import tempfile

    assert "mmx_skinning.hip" in mbuild.SOURCES and mbuild._extra_flags("mmx_skinning.hip", None) == []
    assert "mmx_skin_tables.cpp" in mbuild.SOURCES and mbuild._extra_flags("mmx_skin_tables.cpp", None) == []
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_skinning.hip"),
               "-o", os.path.join(td, "s.o"), "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    kernels = re.split(r"remark: Function Name: ", r.stderr.decode(errors="replace"))[1:]
    names = sorted(k.split()[0] for k in kernels)
    assert len(kernels) == 3 and sum("skinPointsBackwardKernel" in n for n in names) == 1 and sum("skinPointsKernel" in n for n in names) == 2, names
    for k in kernels:
        get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
        fig = {key: get(key) for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill")}
        print(k.split()[0], fig)
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (k.split()[0], fig)
