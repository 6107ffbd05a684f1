"""mmx_closest_points_on_mesh at the C-ABI boundary (no GPU needed): include/mmx.h declares the three entry points with their
parameter lists, the ctypes binding lists them with argument types, and the built library exports them -- a library that
predates the functions lacks the symbols, which is the feature probe (MMX_ABI_VERSION does not move).  The _host form refuses
every bad argument before the first HIP call, and the kernel's translation unit uses no scratch memory."""
import ctypes as C
import os
import re

import numpy as np

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "mmx_closest_points_on_mesh": ["mmx_mesh* mesh", "int32_t batch", "int32_t num_source", "const float* source_dev", "const float* vertices_dev",
                                   "int32_t vertices_shared", "float max_dist", "int32_t* face_index_dev", "float* barycentric_dev", "float* points_dev",
                                   "float* dist2_dev", "void* stream"],
    "mmx_closest_points_on_mesh_host": ["int32_t num_vertices", "int32_t num_triangles", "const int32_t* triangles", "int32_t device", "int32_t batch",
                                        "int32_t num_source", "const float* source_host", "const float* vertices_host", "int32_t vertices_shared",
                                        "float max_dist", "int32_t* face_index_host", "float* barycentric_host", "float* points_host", "float* dist2_host"],
    "mmx_closest_points_on_mesh_plan": ["int32_t batch", "int32_t num_source", "int32_t num_triangles", "int32_t* sources_per_workgroup",
                                        "int32_t* triangle_tile", "int32_t* triangle_ways"],
}  # fmt: skip


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmx.h")).read(), flags=re.S)


def test_declared_in_header_and_bound():
    src = _header()
    for name, want in PARAMS.items():
        m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"include/mmx.h does not declare {name}"
        assert name in capi.SYMBOLS
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == want
        types = _abi.CLOSEST_POINTS_ON_MESH_ARGTYPES[name]
        assert len(types) == len(want), name
        for t, p in zip(types, want):  # floats travel as floats, sizes as int32, host index arrays as int32 pointers, the rest as pointers
            if p.startswith("float "):
                assert t is C.c_float, (name, p)
            elif p.startswith("int32_t "):
                assert t is C.c_int32, (name, p)
            else:
                assert t in (C.c_void_p, _abi.c_int32_p), (name, p)
    assert _abi.MMX_ABI_VERSION == 12
    assert re.search(r"#define\s+MMX_ABI_VERSION\s+12\b", src)


def test_library_exports_them():
    mbuild.build()
    L = capi.lib()
    for name, want in PARAMS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), name
    assert L.mmx_abi_version() == _abi.MMX_ABI_VERSION == 12
    assert "mmx_closest_points_on_mesh.hip" in mbuild.SOURCES and "mmx_closest_points_on_mesh_plan.cpp" in mbuild.SOURCES
    assert "mmx_closest_points_on_mesh_plan.hpp" in mbuild.HEADERS
    p = capi.closest_points_on_mesh_plan(4, 100, 100)
    assert set(p) == {"sources_per_workgroup", "triangle_tile", "triangle_ways"} and all(v >= 1 for v in p.values())
    import momentum_amd
    from momentum_amd import geometry

    assert callable(capi.Mesh.closest_points) and callable(geometry.find_closest_points_on_mesh) and momentum_amd.geometry is geometry
    assert "find_closest_points_on_mesh" in geometry.__all__


def test_host_form_refuses_before_touching_anything():
    """The refusals need no device: they come before the first HIP call, name the function, and leave the outputs alone."""
    mbuild.build()
    L = capi.lib()
    inf = float("inf")
    tri = np.array([[0, 1, 2]], np.int32)
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    src = np.zeros((1, 1, 3), np.float32)
    face = np.full((1, 1), 7, np.int32)
    bary, pts, d2 = np.full((1, 1, 3), -7.25, np.float32), np.full((1, 1, 3), -7.25, np.float32), np.full((1, 1), -7.25, np.float32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    ok = dict(V=3, T=1, tri=tri, batch=1, n=1, source=src, vertices=vtx, max_dist=inf, face=face)
    out_of_range = np.array([[0, 1, 3]], np.int32)
    bad = [dict(V=0), dict(T=0), dict(tri=None), dict(tri=out_of_range), dict(batch=0), dict(n=0), dict(batch=-3), dict(source=None), dict(vertices=None),
           dict(face=None), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(batch=2**31 - 1, n=2**31 - 1)]  # fmt: skip
    for change in bad:
        a = dict(ok, **change)
        rc = L.mmx_closest_points_on_mesh_host(a["V"], a["T"], ip(a["tri"]), 0, a["batch"], a["n"], p(a["source"]), p(a["vertices"]), 0, a["max_dist"],
                                               p(a["face"]), p(bary), p(pts), p(d2))  # fmt: skip
        assert rc == 1, (change, rc)
        assert L.mmx_last_error().decode().startswith("mmx_closest_points_on_mesh_host: "), (change, L.mmx_last_error())
        assert face[0, 0] == 7 and (bary == -7.25).all() and (pts == -7.25).all() and (d2 == -7.25).all(), change
    # the device form's refusals need no device either (a null mesh, and so on, before the first HIP call)
    rc = L.mmx_closest_points_on_mesh(None, 1, 1, p(src), p(vtx), 0, inf, p(face), None, None, None, None)
    assert rc == 1 and L.mmx_last_error().decode().startswith("mmx_closest_points_on_mesh: ") and face[0, 0] == 7


def test_host_form_refuses_without_a_device():
    """Valid arguments and no device to run on -- no GPU at all, or (where there is one) an ordinal far past the last: a
    non-zero status, the failing function's name in mmx_last_error(), and the outputs untouched."""
    mbuild.build()
    L = capi.lib()
    tri = np.array([[0, 1, 2]], np.int32)
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    src = np.full((1, 1, 3), 0.25, np.float32)
    face = np.full((1, 1), 7, np.int32)
    bary, pts, d2 = np.full((1, 1, 3), -7.25, np.float32), np.full((1, 1, 3), -7.25, np.float32), np.full((1, 1), -7.25, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    device = 0 if L.mmx_device_count() <= 0 else 2**20
    rc = L.mmx_closest_points_on_mesh_host(3, 1, tri.ctypes.data_as(C.POINTER(C.c_int32)), device, 1, 1, p(src), p(vtx), 0, float("inf"),
                                           p(face), p(bary), p(pts), p(d2))  # fmt: skip
    msg = L.mmx_last_error().decode()
    assert rc != 0 and msg.startswith(("mmx_closest_points_on_mesh_host: ", "mmx_mesh_create: ")), (rc, msg)
    assert face[0, 0] == 7 and (bary == -7.25).all() and (pts == -7.25).all() and (d2 == -7.25).all()


def test_kernel_is_a_translation_unit_of_its_own_without_scratch():
    """mmx_closest_points_on_mesh.hip is built with the default pipeline; its kernel uses no scratch memory and spills no vector
    register (the VGPR and occupancy figures printed here are the ones DESIGN.md quotes)."""
    import subprocess
    import tempfile

    assert mbuild._extra_flags("mmx_closest_points_on_mesh.hip", None) == []
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_closest_points_on_mesh.hip"),
               "-o", os.path.join(td, "c.o"), "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    kernels = re.split(r"remark: (?:\S+: )?Function Name: ", r.stderr.decode(errors="replace"))[1:]
    names = sorted(k.split()[0] for k in kernels)
    assert len(kernels) == 1 and "closestPointsOnMeshKernel" in names[0], names
    for k in kernels:
        get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
        fig = {key: get(key) for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill")}
        print(k.split()[0], fig)
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (k.split()[0], fig)
