"""mmx_closest_points_on_mesh_plan (no GPU needed): the launch decision the launcher itself takes -- its values are >= 1, the
grid is batch x ceil(N / S) workgroups, and a size below 1 or a grid beyond 2^31 - 1 is refused."""
import ctypes as C

import pytest

from momentum_amd import build as mbuild
from momentum_amd import capi


@pytest.fixture(scope="module", autouse=True)
def _built():
    mbuild.build()


def test_values_are_at_least_one_and_do_not_depend_on_the_sizes():
    first = capi.closest_points_on_mesh_plan(1, 1, 1)
    assert set(first) == {"sources_per_workgroup", "triangle_tile", "triangle_ways"} and all(v >= 1 for v in first.values())
    assert first["triangle_tile"] % (4 * first["triangle_ways"]) == 0  # a wave's share is whole groups of four
    for B, N, T in [(3, 63, 65), (4096, 2000, 4000), (1, 10**6, 10**6)]:
        assert capi.closest_points_on_mesh_plan(B, N, T) == first


def test_grid_arithmetic():
    """The largest batch a source count admits is floor((2^31 - 1) / ceil(N / S)): one more is refused."""
    S = capi.closest_points_on_mesh_plan(1, 1, 1)["sources_per_workgroup"]
    for N in (1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 1000 * S + 1):
        groups = -(-N // S)
        most = (2**31 - 1) // groups
        capi.closest_points_on_mesh_plan(most, N, 7)
        if most < 2**31 - 1:
            with pytest.raises(capi.MmxError, match="mmx_closest_points_on_mesh_plan"):
                capi.closest_points_on_mesh_plan(most + 1, N, 7)


def test_refusals():
    for B, N, T in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5), (2**31 - 1, 2**31 - 1, 1)]:
        with pytest.raises(capi.MmxError, match="mmx_closest_points_on_mesh_plan") as e:
            capi.closest_points_on_mesh_plan(B, N, T)
        assert e.value.code == 1
    L = capi.lib()
    s = C.c_int32(-5)
    assert L.mmx_closest_points_on_mesh_plan(0, 1, 1, C.byref(s), None, None) == 1 and s.value == -5  # nothing is written on a refusal
    assert L.mmx_closest_points_on_mesh_plan(1, 1, 1, None, None, None) == 0  # any output may be NULL
