"""mmx_closest_points_plan, the launch decision of mmx_closest_points as a pure host function (no GPU): refusals, monotony,
and that the parity shape list of tests/closest_points_reference.py reaches every distinct plan the function returns (today
one per kernel instantiation: the function has no switch-over between forms) and every edge the plan names."""
import itertools

import pytest

from momentum_amd import build as mbuild
from momentum_amd import capi
from tests import closest_points_reference as ref


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def _plan(B, N, M, normals=False):
    p = capi.closest_points_plan(B, N, M, normals)
    return p["sources_per_workgroup"], p["target_tile"], p["target_ways"]


def test_refuses_bad_sizes():
    for B, N, M in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5), (2**31 - 1, 2**31 - 1, 1)]:
        with pytest.raises(capi.MmxError) as e:
            capi.closest_points_plan(B, N, M)
        assert e.value.code == 1
    assert capi.lib().mmx_closest_points_plan(1, 1, 1, 0, None, None, None) == 0  # any output may be NULL
    _plan(2**31 - 1, 1, 2**31 - 1)  # the largest grid that is allowed


def test_plan_is_sane_and_monotone():
    sizes = [1, 2, 63, 64, 255, 256, 257, 1023, 1024, 1025, 5000, 100000]
    batches = [1, 2, 3, 255, 256, 1023, 1024, 1025, 4096, 65536]
    for normals in (False, True):
        for M in (1, 2000):
            last_n = {}
            for B in batches:
                prev = None
                for N in sizes:
                    S, T, W = _plan(B, N, M, normals)
                    assert S % 64 == 0 and T % (4 * W) == 0 and W in (1, 4) and S >= 64 and T >= 4
                    assert (S, T, W) == _plan(B, N, 1, normals), "the plan does not depend on the number of targets"
                    if prev is not None:  # more sources: never fewer sources per workgroup, never more ways
                        assert S >= prev[0] and W <= prev[2] and T == prev[1]
                    if N in last_n:  # a larger batch likewise
                        assert S >= last_n[N][0] and W <= last_n[N][2]
                    prev = last_n[N] = (S, T, W)
    assert _plan(4, 100, 100, True)[1] <= _plan(4, 100, 100, False)[1]  # the normals share the tile's LDS


def test_parity_shapes_reach_every_plan_and_every_edge():
    for normals in (False, True):
        shapes = ref.parity_shapes(capi.closest_points_plan, normals)
        reached = {_plan(B, N, M, normals) for B, N, M in shapes}
        # every plan of the sizes up to 2^15 (far beyond the list's largest; the plan is piecewise constant: powers of two and
        # their neighbours cover its pieces)
        grid = sorted({v for k in range(0, 16) for v in (2**k - 1, 2**k, 2**k + 1) if v >= 1})
        every = {_plan(B, N, 1, normals) for B, N in itertools.product(grid, grid)}
        assert every == reached, (every, reached)
        assert max(N * M for _, N, M in shapes) <= 1_100_000 and max(B for B, _, _ in shapes) <= 8  # about 10^6 pairs, a handful of instances
        (S, T, W), = reached
        for n in (S - 1, S, S + 1):
            assert any(s[1] == n for s in shapes)
        for m in (T - 1, T, T + 1, 2 * T + 1):
            assert any(s[2] == m for s in shapes)
        if W > 1:
            assert any(s[2] == W - 1 for s in shapes) and any(s[2] == W + 1 for s in shapes)
        for fixed in [(1, 1, 1), (3, 63, 65), (2, 64, 64), (2, 65, 1)]:
            assert fixed in shapes
