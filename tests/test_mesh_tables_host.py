"""The vertex-sorted incidence list of the vertex-normal kernels (mmx_host_mesh_tables: buildMeshTables in
momentum_amd/csrc/mmx_mesh_tables.cpp) on the CPU, bit for bit against a NumPy lexsort: every (triangle, corner) pair sorted
by (vertex, triangle, corner), vertex_start [V + 1] its index, and the largest valence -- and the refusals of the table
function.  The per-wave layout the kernels read, which that function does not return, is checked by a stand-alone C++ program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from momentum_amd import _abi, capi, make_test_mesh
from momentum_amd import build as mbuild
from tests import vertex_normals_reference as ref

MMX_ERR_INVALID_ARGUMENT = 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _expected(V, tri):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    t, c = np.divmod(np.arange(tri.size), 3)
    v = tri.reshape(-1)
    order = np.lexsort((c, t, v))  # (last key first: vertex, then triangle, then corner)
    count = np.bincount(v, minlength=V)
    return np.concatenate([[0], np.cumsum(count)]).astype(np.int32), t[order].astype(np.int32), c[order].astype(np.int32), int(count.max())


def _check(V, tri):
    got = capi.host_mesh_tables(V, tri)
    start, et, ec, valence = _expected(V, tri)
    assert np.array_equal(got["vertex_start"], start) and got["vertex_start"].dtype == np.int32
    assert np.array_equal(got["entry_triangle"], et) and np.array_equal(got["entry_corner"], ec)
    assert got["max_valence"] == valence
    return got


def test_torus():
    m = make_test_mesh(8, 4, 0.1, 1)
    got = _check(32, m.triangles)
    assert got["max_valence"] == 6 and np.all(np.diff(got["vertex_start"]) == 6) and len(got["entry_triangle"]) == 3 * 64
    _check(2048, make_test_mesh(64, 32, 0.1, 2).triangles)


def test_fan_with_a_hub_of_valence_1000():
    _, tri = ref.MESHES["fan_1000"]()
    got = _check(1002, tri)
    assert got["max_valence"] == 1000 and got["vertex_start"][1] == 1000
    assert np.array_equal(got["entry_triangle"][:1000], np.arange(1000)) and not got["entry_corner"][:1000].any()


def test_isolated_vertices():
    tri = make_test_mesh(10, 6, 0.1, 3).triangles
    got = _check(65, tri)  # 60 on the grid, five of no triangle
    assert np.all(got["vertex_start"][60:] == 3 * len(tri))
    got = _check(7, [[5, 3, 1]])  # isolated vertices first, last and in between
    assert got["vertex_start"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert got["entry_triangle"].tolist() == [0, 0, 0] and got["entry_corner"].tolist() == [2, 1, 0]


def test_a_vertex_at_two_corners_of_one_triangle():
    got = _check(3, [[1, 1, 2], [2, 0, 2], [0, 0, 0]])
    s = got["vertex_start"]
    assert list(zip(got["entry_triangle"][s[1] : s[2]], got["entry_corner"][s[1] : s[2]])) == [(0, 0), (0, 1)]
    assert list(zip(got["entry_triangle"][s[0] : s[1]], got["entry_corner"][s[0] : s[1]])) == [(1, 1), (2, 0), (2, 1), (2, 2)]
    assert got["max_valence"] == 4


def test_one_triangle():
    got = _check(3, [[2, 0, 1]])
    assert got["vertex_start"].tolist() == [0, 1, 2, 3] and got["entry_corner"].tolist() == [1, 2, 0] and got["max_valence"] == 1


def test_any_output_may_be_null():
    L = capi.lib()
    tri = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    n, mv = C.c_int32(0), C.c_int32(0)
    assert L.mmx_host_mesh_tables(4, 2, _abi.as_ptr(tri, C.c_int32), None, None, None, C.byref(n), C.byref(mv)) == 0
    assert (n.value, mv.value) == (6, 2)
    assert L.mmx_host_mesh_tables(4, 2, _abi.as_ptr(tri, C.c_int32), None, None, None, None, None) == 0


def test_layout_under_sanitizers(tmp_path):
    """What mmx_host_mesh_tables does not return -- the records per group of 64 vertices -- checked where it is built: a
    stand-alone program (tests/cpp/test_mesh_tables.cpp) that links mmx_mesh_tables.cpp and nothing else."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = [os.path.join(root, "tests", "cpp", "test_mesh_tables.cpp"), os.path.join(root, "momentum_amd", "csrc", "mmx_mesh_tables.cpp")]
    exe = str(tmp_path / "test_mesh_tables")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout


def test_refusals():
    L = capi.lib()
    start, et, ec = np.zeros(5, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int32)
    n, mv = C.c_int32(-5), C.c_int32(-5)
    ip = lambda a: _abi.as_ptr(a, C.c_int32)

    def call(V, tri, T=None):
        t = None if tri is None else np.ascontiguousarray(tri, np.int32)
        return L.mmx_host_mesh_tables(V, (0 if t is None else len(t)) if T is None else T, None if t is None else ip(t), ip(start), ip(et), ip(ec), C.byref(n), C.byref(mv))

    ok = [[0, 1, 2], [2, 1, 3]]
    assert call(4, ok) == 0 and n.value == 6 and mv.value == 2
    n.value, mv.value, start[:] = -5, -5, 0
    for V, tri, T, word in ((4, [[0, 1, 4], [2, 1, 3]], None, "out of range"), (4, [[0, 1, 2], [2, -1, 3]], None, "out of range"), (0, ok, None, ">= 1"),
                            (-3, ok, None, ">= 1"), (4, ok, 0, ">= 1"), (4, ok, -1, ">= 1"), (4, None, 2, "null"), (4, ok, 2**30, "2^31")):  # fmt: skip
        assert call(V, tri, T) == MMX_ERR_INVALID_ARGUMENT, (V, tri, T)
        msg = L.mmx_last_error().decode()
        assert msg.startswith("mmx_host_mesh_tables: ") and word in msg, msg
    assert n.value == -5 and mv.value == -5 and not start.any()  # a refusal writes nothing
