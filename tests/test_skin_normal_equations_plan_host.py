"""The split of mmx_skin_normal_equations_split as the library decides it (no GPU needed;
momentum_amd/csrc/mmx_skin_normal_equations_plan.cpp through the exported queries): the workspace size and the plan of
parts = 0, and the part ranges as the library reports them (mmx_skin_normal_equations_part_range: the function the kernel's
tile loop takes its range from) -- they tile [0, T) without gap or overlap and are floor(p T / Pe), Pe = min(parts, T)."""
import ctypes as C
import itertools

import pytest

from momentum_amd import _abi
from momentum_amd import build as mbuild
from momentum_amd import capi

POSITION, PLANE = _abi.MMX_VC_POSITION, _abi.MMX_VC_PLANE


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def test_part_ranges_tile_the_tiles_without_gap_or_overlap():
    rng = capi.skin_normal_equations_part_range
    for T in range(1, 71):
        for parts in list(range(1, 71)) + [512]:
            pe = rng(T, parts, 0)[2]
            assert pe == min(parts, T)
            r = [rng(T, parts, p) for p in range(pe)]
            assert all(x[2] == pe for x in r)
            assert r[0][0] == 0 and r[-1][1] == T
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))  # no gap, no overlap
            assert all(hi > lo for lo, hi, _ in r)  # no part is empty
            assert [x[0] for x in r] == [p * T // pe for p in range(pe)]  # the rule of include/mmx.h
    assert rng(201326592, 512, 511)[:2] == (511 * 201326592 // 512, 201326592)  # the largest tile count: no 32-bit overflow
    L = capi.lib()
    for T, parts, p in [(0, 1, 0), (-3, 2, 0), (5, 0, 0), (5, 513, 0), (5, -1, 0), (5, 3, 3), (5, 3, -1), (2, 7, 2)]:
        b = C.c_int32(-5)
        assert L.mmx_skin_normal_equations_part_range(T, parts, p, C.byref(b), None, None) == 1 and b.value == -5, (T, parts, p)
    assert L.mmx_skin_normal_equations_part_range(5, 3, 2, None, None, None) == 0  # any output may be NULL


def test_workspace_bytes():
    wb = capi.skin_normal_equations_workspace_bytes
    for B, n in [(1, 1), (3, 33), (16, 128)]:
        assert wb(B, n, 0) == 0 and wb(B, n, 1) == 0
        assert wb(B, n, 2) > 0 and wb(B, n, 2) % 16 == 0
    # room for what a part stores: the accumulators of the lower block triangle, a double per padded column, the error
    for n in (1, 32, 33, 64, 65, 96, 97, 128):
        nb = (n + 31) // 32
        assert wb(1, n, 2) >= 2 * (nb * (nb + 1) // 2 * 1024 * 4 + 32 * nb * 8 + 8)
    # does not decrease in any argument
    Bs, ns, ps = (1, 2, 3, 16, 257, 4096), (1, 5, 32, 33, 64, 65, 127, 128), (0, 1, 2, 3, 4, 7, 64, 511, 512)
    for (B0, B1), n, p in itertools.product(zip(Bs, Bs[1:]), ns, ps):
        assert wb(B0, n, p) <= wb(B1, n, p)
    for B, (n0, n1), p in itertools.product(Bs, zip(ns, ns[1:]), ps):
        assert wb(B, n0, p) <= wb(B, n1, p)
    for B, n, (p0, p1) in itertools.product(Bs, ns, zip(ps, ps[1:])):
        assert wb(B, n, p0) <= wb(B, n, p1)
    for B, n, p in [(0, 5, 2), (-1, 5, 2), (1, 0, 2), (1, 129, 2), (1, -3, 2), (1, 5, -1), (1, 5, 513), (0, 5, 1), (1, 0, 0)]:
        assert wb(B, n, p) == -1, (B, n, p)
    assert wb(2**31 - 1, 128, 512) > 2**40  # no overflow at the largest arguments


def _tiles(plane, count):
    rows = count if plane else 3 * count
    return -(-rows // 32)


def test_plan():
    plan = capi.skin_normal_equations_plan
    counts = (1, 10, 11, 85, 86, 171, 300, 2000, 20000, 10**6)
    for plane, cu, wpc in itertools.product((False, True), (1, 64, 256, 304), (1, 2)):
        for count in counts:
            T = _tiles(plane, count)
            for B in (1, 2, 3, 16, 17, 255, 256, 257, 512, 513, 4096):
                p = plan(B, count, plane=plane, compute_units=cu, workgroups_per_cu=wpc)
                assert 1 <= p <= min(T, 512, max(1, cu * wpc // B)), (plane, cu, wpc, count, B, p)
                if B >= cu * wpc:
                    assert p == 1
        for B in (1, 3, 16, 300):  # does not decrease as count grows
            ps = [plan(B, c, plane=plane, compute_units=cu, workgroups_per_cu=wpc) for c in counts]
            assert ps == sorted(ps), (B, ps)
        for count in counts:  # does not increase as batch grows
            ps = [plan(B, count, plane=plane, compute_units=cu, workgroups_per_cu=wpc) for B in (1, 2, 3, 16, 100, 256, 512, 4096)]
            assert ps == sorted(ps, reverse=True), (count, ps)
    # the shapes of the rate script (20 000 position constraints are 1875 tiles, 2 000 are 188)
    assert plan(16, 20000, plane=False, compute_units=256, workgroups_per_cu=2) == 32
    assert plan(256, 2000, plane=False, compute_units=256, workgroups_per_cu=2) == 2
    assert plan(4096, 2000, plane=False, compute_units=256, workgroups_per_cu=2) == 1


def test_plan_refusals_write_nothing():
    L = capi.lib()
    for B, type_, count, cu, wpc in [(0, POSITION, 5, 256, 2), (-1, PLANE, 5, 256, 2), (1, POSITION, 0, 256, 2), (1, PLANE, -4, 256, 2),
                                     (1, 2, 5, 256, 2), (1, -1, 5, 256, 2), (1, POSITION, 5, 0, 2), (1, POSITION, 5, -256, 2), (1, POSITION, 5, 256, 0)]:  # fmt: skip
        out = C.c_int32(-5)
        assert L.mmx_skin_normal_equations_plan(B, type_, count, cu, wpc, C.byref(out)) == 1 and out.value == -5
        assert L.mmx_last_error().decode().startswith("mmx_skin_normal_equations_plan: ")
    with pytest.raises(capi.MmxError, match="mmx_skin_normal_equations_plan"):
        capi.skin_normal_equations_plan(0, 5, plane=True, compute_units=256)
    assert L.mmx_skin_normal_equations_plan(1, PLANE, 5, 256, 2, None) == 0  # the output may be NULL
