"""mmx_closest_points at the C-ABI boundary (no GPU needed): include/mmx.h declares the three entry points with their
parameter lists, the ctypes binding lists them with argument types, and the built library exports them -- a library that
predates the functions lacks the symbols, which is the feature probe (MMX_ABI_VERSION does not move)."""
import ctypes as C
import os
import re

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMMON = ["int32_t batch", "int32_t num_source", "int32_t num_target"]
PARAMS = {
    "mmx_closest_points": _COMMON + ["const float* source_dev", "const float* target_dev", "int32_t target_shared", "const float* source_normals_dev",
                                     "const float* target_normals_dev", "float max_dist", "float min_normal_dot", "int32_t* index_dev", "float* dist2_dev",
                                     "float* points_dev", "void* stream"],
    "mmx_closest_points_host": _COMMON + ["const float* source_host", "const float* target_host", "int32_t target_shared", "const float* source_normals_host",
                                          "const float* target_normals_host", "float max_dist", "float min_normal_dot", "int32_t* index_host",
                                          "float* dist2_host", "float* points_host"],
    "mmx_closest_points_plan": _COMMON + ["int32_t with_normals", "int32_t* sources_per_workgroup", "int32_t* target_tile", "int32_t* target_ways"],
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
    assert _abi.MMX_ABI_VERSION == 12
    assert re.search(r"#define\s+MMX_ABI_VERSION\s+12\b", src)
    assert len(_abi.CLOSEST_POINTS_ARGTYPES) == len(PARAMS["mmx_closest_points"])
    assert len(_abi.CLOSEST_POINTS_PLAN_ARGTYPES) == len(PARAMS["mmx_closest_points_plan"])
    for i, p in enumerate(PARAMS["mmx_closest_points"]):  # the two floats travel as floats, the sizes as int32, the rest as pointers
        want = C.c_float if p.startswith("float ") else (C.c_int32 if p.startswith("int32_t ") else C.c_void_p)
        assert _abi.CLOSEST_POINTS_ARGTYPES[i] is want, p


def test_library_exports_them():
    mbuild.build()
    L = capi.lib()
    for name, want in PARAMS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), name
    assert L.mmx_abi_version() == _abi.MMX_ABI_VERSION == 12
    assert "mmx_closest_points.hip" in mbuild.SOURCES and "mmx_closest_points_plan.cpp" in mbuild.SOURCES
    p = capi.closest_points_plan(4, 100, 100)
    assert set(p) == {"sources_per_workgroup", "target_tile", "target_ways"} and all(v >= 1 for v in p.values())
    import momentum_amd
    from momentum_amd import geometry

    assert callable(capi.closest_points) and callable(geometry.find_closest_points) and momentum_amd.geometry is geometry


def test_host_form_refuses_before_touching_anything():
    """The refusals need no device: they come before the first HIP call."""
    mbuild.build()
    L = capi.lib()
    inf = float("inf")
    src = (C.c_float * 3)(0, 0, 0)
    idx = (C.c_int32 * 1)(7)
    ok = dict(batch=1, n=1, m=1, source=src, target=src, sn=None, tn=None, max_dist=inf, min_dot=0.0, index=idx)
    bad = [dict(batch=0), dict(n=0), dict(m=0), dict(source=None), dict(target=None), dict(index=None), dict(max_dist=-1.0), dict(max_dist=float("nan")),
           dict(sn=src), dict(tn=src), dict(sn=src, tn=src, min_dot=float("nan")), dict(batch=2**31 - 1, n=2**31 - 1)]  # fmt: skip
    for change in bad:
        a = dict(ok, **change)
        rc = L.mmx_closest_points_host(a["batch"], a["n"], a["m"], a["source"], a["target"], 0, a["sn"], a["tn"], a["max_dist"], a["min_dot"], a["index"], None, None)
        assert rc == 1, (change, rc)
        assert L.mmx_last_error().decode().startswith("mmx_closest_points_host: "), change
        assert idx[0] == 7


def test_kernels_are_a_translation_unit_of_their_own_without_scratch():
    """mmx_closest_points.hip is built with the default pipeline; both instantiations of the kernel use no scratch memory and
    spill no vector register."""
    import subprocess
    import tempfile

    assert mbuild._extra_flags("mmx_closest_points.hip", None) == []
    with tempfile.TemporaryDirectory() as td:
        cmd = [mbuild._hipcc(), f"--offload-arch={mbuild.ARCH}", "-O3", "-std=c++17", "-c", os.path.join(mbuild.CSRC, "mmx_closest_points.hip"),
               "-o", os.path.join(td, "c.o"), "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    kernels = re.split(r"remark: Function Name: ", r.stderr.decode(errors="replace"))[1:]
    names = sorted(k.split()[0] for k in kernels)
    assert len(kernels) == 2 and all("closestPointsKernel" in n for n in names), names
    for k in kernels:
        get = lambda key: int(re.search(re.escape(key) + r":? (\d+)", k).group(1))
        fig = {key: get(key) for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill")}
        print(k.split()[0], fig)
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, (k.split()[0], fig)
