"""The joint-sorted influence list of the skinning backward pass (mmx_host_skin_tables: buildSkinTables in
momentum_amd/csrc/mmx_skin_tables.cpp) on the CPU, bit for bit against a NumPy lexsort: every (vertex, slot) pair with a
non-zero weight sorted by (joint, vertex, slot), joint_start [J + 1] its index -- and the refusals of the table function.  The
wave partition and the entry weights, which that function does not return, are checked by a stand-alone C++ program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from momentum_amd import _abi, capi
from momentum_amd import build as mbuild
from tests import skinning_reference as ref

MMX_ERR_INVALID_ARGUMENT = 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _expected(J, joint, weight):
    joint, weight = np.asarray(joint), np.asarray(weight)
    v, k = np.nonzero(weight != 0)
    j = joint[v, k]
    order = np.lexsort((k, v, j))  # (last key first: joint, then vertex, then slot)
    start = np.concatenate([[0], np.cumsum(np.bincount(j, minlength=J))]).astype(np.int32)
    return start, v[order].astype(np.int32), k[order].astype(np.int32)


def _check(J, joint, weight):
    got = capi.host_skin_tables(J, joint, weight)
    start, ev, es = _expected(J, joint, weight)
    assert np.array_equal(got["joint_start"], start)
    assert np.array_equal(got["entry_vertex"], ev) and np.array_equal(got["entry_slot"], es)
    return got


def test_three_joints_with_padding_and_a_joint_without_influences():
    joint, weight, _ = ref.hand_skin("character3_k4")
    got = _check(3, joint, weight)
    assert got["joint_start"][2] == got["joint_start"][3] == len(got["entry_vertex"]) == 12  # joint 2: only zero-weight slots name it


def test_one_vertex_one_slot():
    got = _check(1, [[0]], [[1.0]])
    assert got["joint_start"].tolist() == [0, 1] and got["entry_vertex"].tolist() == [0] and got["entry_slot"].tolist() == [0]


def test_all_vertices_on_joint_zero():
    got = _check(3, np.zeros((1000, 1), np.int32), np.ones((1000, 1), np.float32))
    assert got["joint_start"].tolist() == [0, 1000, 1000, 1000] and np.array_equal(got["entry_vertex"], np.arange(1000))


def test_eight_slots_with_a_joint_repeated_in_one_vertex():
    rng = np.random.default_rng(3)
    joint = rng.integers(0, 5, size=(40, 8)).astype(np.int32)
    weight = rng.uniform(0.1, 1.0, size=(40, 8)).astype(np.float32)
    weight[rng.uniform(size=(40, 8)) < 0.3] = 0.0
    joint[7] = [4, 1, 4, 0, 2, 3, 1, 0]  # joint 4 in slots 0 and 2, joint 1 in 1 and 6: every entry kept, in slot order
    weight[7] = 0.125
    got = _check(5, joint, weight)
    s = got["joint_start"]
    on4 = [(v, k) for v, k in zip(got["entry_vertex"][s[4] : s[5]], got["entry_slot"][s[4] : s[5]]) if v == 7]
    assert on4 == [(7, 0), (7, 2)]


def test_negative_zero_weight_is_padding_and_a_tiny_one_is_not():
    _check(2, [[0, 1, 1]], np.array([[-0.0, 1e-45, 0.5]], np.float32))


def test_wave_partition_and_entry_weights_under_sanitizers(tmp_path):
    """What mmx_host_skin_tables does not return -- waveStart and entryWeight -- checked where it is built: a stand-alone
    program (tests/cpp/test_skin_tables.cpp) that links mmx_skin_tables.cpp and nothing else."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = [os.path.join(root, "tests", "cpp", "test_skin_tables.cpp"), os.path.join(root, "momentum_amd", "csrc", "mmx_skin_tables.cpp")]
    exe = str(tmp_path / "test_skin_tables")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout


def test_refusals():
    L = capi.lib()
    start, ev, es = np.zeros(4, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int32)
    n = C.c_int32(-5)
    ip = lambda a: _abi.as_ptr(a, C.c_int32)

    def call(J, joint, weight, K=None, V=None):
        jt, wt = np.ascontiguousarray(joint, np.int32), np.ascontiguousarray(weight, np.float32)
        d = _abi.SkinDesc(jt.shape[0] if V is None else V, jt.shape[1] if K is None else K, ip(jt), _abi.as_ptr(wt, C.c_float), _abi.c_float_p(), _abi.c_float_p())
        return L.mmx_host_skin_tables(J, C.byref(d), ip(start), ip(ev), ip(es), C.byref(n))

    ok_j, ok_w = [[0, 1], [2, 0]], [[0.5, 0.5], [1.0, 0.0]]
    assert call(3, ok_j, ok_w) == 0 and n.value == 3
    n.value, start[:] = -5, 0
    assert call(3, [[0, 3], [2, 0]], ok_w) == MMX_ERR_INVALID_ARGUMENT  # joint out of range
    assert "out of range" in L.mmx_last_error().decode()
    assert call(3, [[0, 1], [2, -1]], ok_w) == MMX_ERR_INVALID_ARGUMENT  # ... in a zero-weight slot too
    assert call(3, ok_j, ok_w, K=0) == MMX_ERR_INVALID_ARGUMENT
    assert call(3, np.zeros((1, 9), np.int32), np.ones((1, 9), np.float32)) == MMX_ERR_INVALID_ARGUMENT  # K = 9
    assert call(3, ok_j, ok_w, V=0) == MMX_ERR_INVALID_ARGUMENT
    assert call(3, ok_j, [[0.5, np.inf], [1.0, 0.0]]) == MMX_ERR_INVALID_ARGUMENT
    assert L.mmx_host_skin_tables(3, None, ip(start), ip(ev), ip(es), C.byref(n)) == MMX_ERR_INVALID_ARGUMENT
    d = _abi.SkinDesc(2, 2, _abi.c_int32_p(), _abi.c_float_p(), _abi.c_float_p(), _abi.c_float_p())
    assert L.mmx_host_skin_tables(3, C.byref(d), ip(start), ip(ev), ip(es), C.byref(n)) == MMX_ERR_INVALID_ARGUMENT  # null arrays
    assert n.value == -5 and not start.any()  # a refusal writes nothing
