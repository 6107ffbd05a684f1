"""mmx_vertex_normals at the C-ABI boundary (no GPU needed): include/mmx.h declares the entry points with their parameter
lists, the ctypes binding lists them with argument types, and the built library exports them -- a library that predates the
functions lacks the symbols, which is the feature probe (MMX_ABI_VERSION does not move).  The refusals of mmx_mesh_create and
of the _host forms come before the first HIP call, and the kernels' translation unit uses no scratch memory."""
import ctypes as C
import os
import re

import numpy as np

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MESH = ["int32_t num_vertices", "int32_t num_triangles", "const int32_t* triangles", "int32_t device"]
PARAMS = {
    "mmx_mesh_create": _MESH + ["mmx_mesh** out"],
    "mmx_mesh_destroy": ["mmx_mesh* mesh"],
    "mmx_mesh_num_vertices": ["const mmx_mesh* mesh"],
    "mmx_mesh_num_triangles": ["const mmx_mesh* mesh"],
    "mmx_vertex_normals": ["mmx_mesh* mesh", "int32_t batch", "const float* positions_dev", "float* normals_dev", "float* sums_dev", "void* stream"],
    "mmx_vertex_normals_backward": ["mmx_mesh* mesh", "int32_t batch", "const float* positions_dev", "const float* sums_dev", "const float* normal_grad_dev",
                                    "float* position_grad_dev", "void* stream"],
    "mmx_vertex_normals_host": _MESH + ["int32_t batch", "const float* positions_host", "float* normals_host", "float* sums_host"],
    "mmx_vertex_normals_backward_host": _MESH + ["int32_t batch", "const float* positions_host", "const float* sums_host", "const float* normal_grad_host",
                                                 "float* position_grad_host"],
    "mmx_host_mesh_tables": ["int32_t num_vertices", "int32_t num_triangles", "const int32_t* triangles", "int32_t* vertex_start", "int32_t* entry_triangle",
                             "int32_t* entry_corner", "int32_t* num_entries", "int32_t* max_valence"],
}  # fmt: skip
MMX_ERR_INVALID_ARGUMENT = 1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmx.h")).read(), flags=re.S)


def test_declared_in_header_and_bound():
    src = _header()
    for name, want in PARAMS.items():
        m = re.search(r"\b(?:int32_t|void)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"include/mmx.h does not declare {name}"
        assert name in capi.SYMBOLS
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == want
        assert len(_abi.MESH_ARGTYPES[name]) == len(want), name
        for p, t in zip(want, _abi.MESH_ARGTYPES[name]):  # sizes travel as int32, everything else as a pointer
            assert (t is C.c_int32) == p.startswith("int32_t "), (name, p)
    assert set(PARAMS) == set(_abi.MESH_ARGTYPES)
    assert re.search(r"typedef\s+struct\s+mmx_mesh\s+mmx_mesh\s*;", src)
    assert _abi.MMX_ABI_VERSION == 12
    assert re.search(r"#define\s+MMX_ABI_VERSION\s+12\b", src)


def test_library_exports_them():
    mbuild.build()
    L = capi.lib()
    for name, want in PARAMS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), name
    assert L.mmx_abi_version() == _abi.MMX_ABI_VERSION == 12
    for f in ("mmx_vertex_normals.hip", "mmx_mesh_tables.cpp"):
        assert f in mbuild.SOURCES and os.path.exists(os.path.join(mbuild.CSRC, f))
    assert "mmx_mesh_tables.hpp" in mbuild.HEADERS
    assert L.mmx_mesh_num_vertices(None) == 0 and L.mmx_mesh_num_triangles(None) == 0
    L.mmx_mesh_destroy(None)  # (a null handle is fine)
    import momentum_amd
    from momentum_amd import autograd, geometry

    assert callable(capi.Mesh) and callable(capi.host_mesh_tables) and callable(autograd.vertex_normals)
    assert callable(geometry.compute_vertex_normals) and "compute_vertex_normals" in geometry.__all__
    for name in ("make_test_mesh", "make_test_skinned_mesh"):
        assert name in momentum_amd.__all__ and callable(getattr(momentum_amd, name))


def _refused(L, rc, name):
    assert rc == MMX_ERR_INVALID_ARGUMENT, (name, rc)
    assert L.mmx_last_error().decode().startswith(name + ": "), (name, L.mmx_last_error())


def test_create_and_device_forms_refuse_before_the_first_hip_call():
    """No device is needed: a refusal comes before the first HIP call (on a machine without a GPU a HIP call would fail
    with another status)."""
    mbuild.build()
    L = capi.lib()
    tri = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    tp = _abi.as_ptr(tri, C.c_int32)
    h = C.c_void_p(0)
    bad_tri = np.array([[0, 1, 2], [2, 4, 3]], np.int32)
    neg_tri = np.array([[0, -1, 2], [2, 1, 3]], np.int32)
    for V, T, t, out in ((4, 2, tp, None), (0, 2, tp, C.byref(h)), (-1, 2, tp, C.byref(h)), (4, 0, tp, C.byref(h)), (4, 2, None, C.byref(h)),
                         (4, 2, _abi.as_ptr(bad_tri, C.c_int32), C.byref(h)), (4, 2, _abi.as_ptr(neg_tri, C.c_int32), C.byref(h)),
                         (4, 2**30, tp, C.byref(h))):  # fmt: skip
        _refused(L, L.mmx_mesh_create(V, T, t, 0, out), "mmx_mesh_create")
        assert not h.value
    # the device forms without a handle (what a handle would add is checked on the GPU)
    buf = np.full(12, -7.25, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    _refused(L, L.mmx_vertex_normals(None, 1, p, p, None, None), "mmx_vertex_normals")
    _refused(L, L.mmx_vertex_normals_backward(None, 1, p, p, p, p, None), "mmx_vertex_normals_backward")
    assert np.all(buf == -7.25)


def test_host_forms_refuse_before_touching_anything():
    mbuild.build()
    L = capi.lib()
    tri = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    bad_tri = np.array([[0, 1, 2], [2, 1, 4]], np.int32)
    pos = np.zeros((1, 4, 3), np.float32)
    out, sums, grad = (np.full((1, 4, 3), -7.25, np.float32) for _ in range(3))
    fp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ip = lambda a: None if a is None else _abi.as_ptr(a, C.c_int32)
    ok = dict(V=4, T=2, tri=tri, batch=1, pos=pos, out=out, sums=sums, grad=grad)
    common = [dict(V=0), dict(V=-4), dict(T=0), dict(tri=None), dict(tri=bad_tri), dict(T=2**30), dict(batch=0), dict(batch=-1), dict(pos=None),
              dict(batch=2**31 - 1), dict(V=2**31 - 1, batch=2**31 - 1), dict(V=2**28, batch=3)]  # fmt: skip
    for change in common + [dict(out=None)]:
        a = dict(ok, **change)
        rc = L.mmx_vertex_normals_host(a["V"], a["T"], ip(a["tri"]), 0, a["batch"], fp(a["pos"]), fp(a["out"]), fp(a["sums"]))
        _refused(L, rc, "mmx_vertex_normals_host")
    for change in common + [dict(sums=None), dict(grad=None), dict(out=None)]:
        a = dict(ok, **change)
        rc = L.mmx_vertex_normals_backward_host(a["V"], a["T"], ip(a["tri"]), 0, a["batch"], fp(a["pos"]), fp(a["sums"]), fp(a["grad"]), fp(a["out"]))
        _refused(L, rc, "mmx_vertex_normals_backward_host")
    assert all(np.all(x == -7.25) for x in (out, sums, grad))


def test_kernels_are_a_translation_unit_of_their_own_without_scratch():
    """mmx_vertex_normals.hip is built with the default pipeline; both kernels use no scratch memory and spill no vector
    register."""
    import subprocess
    import tempfile

    assert mbuild._extra_flags("mmx_vertex_normals.hip", None) == [] and mbuild._extra_flags("mmx_mesh_tables.cpp", None) == []
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_vertex_normals.hip"),
               "-o", os.path.join(td, "c.o"), "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    kernels = re.split(r"remark: Function Name: ", r.stderr.decode(errors="replace"))[1:]
    names = sorted(k.split()[0] for k in kernels)
    assert len(kernels) == 2 and "vertexNormalsBackwardKernel" in names[1] and "vertexNormalsKernel" in names[0], names
    for k in kernels:
        get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
        fig = {key: get(key) for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill")}
        print(k.split()[0], fig)
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (k.split()[0], fig)
