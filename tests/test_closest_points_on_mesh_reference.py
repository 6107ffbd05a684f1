"""The acceptance rule of mmx_closest_points_on_mesh on the CPU (no GPU needed): the float32 restatement of the record and the
pair passes the rule on every parity case, within a quarter of K (which is how K is defined); the same restatement with d2
from the expanded quadratic fails it on the near-surface sources; the analytic cases; and the max_dist values of the GPU
test leave no source undecided."""
import numpy as np
import pytest

from momentum_amd import build as mbuild
from momentum_amd import capi
from tests import closest_points_on_mesh_reference as ref


@pytest.fixture(scope="module")
def shapes():
    mbuild.build()
    return ref.parity_shapes(capi.closest_points_on_mesh_plan)


def _cases(shapes):
    for B, N, T in shapes:
        for shared in (True, False):
            yield (B, N, T, shared), ref.parity_case(B, N, T, shared)
    yield ref.OFFSET_SHAPE + (False,), ref.parity_case(*ref.OFFSET_SHAPE, False, offset=(100.0, 100.0, 100.0))


def test_restatement_passes_the_rule_and_defines_k(shapes):
    worst = dict(worst_choice=0.0, worst_dist=0.0, worst_weights=0.0, worst_sum_u=0.0)
    for key, c in _cases(shapes):
        face, bary, points, dist2 = ref.restatement32(c["source"], c["vertices"], c["triangles"])
        st = ref.check(c["source"], c["vertices"], c["triangles"], face, bary, points, dist2)
        assert st["valid"] == st["sources"] and st["undecided"] == 0, key
        for k in worst:
            worst[k] = max(worst[k], st[k])
    print("restatement32 worst figures (u R):", worst, "K =", ref.K)
    assert max(worst["worst_choice"], worst["worst_dist"], worst["worst_weights"]) <= ref.RESTATEMENT_BOUND  # K is 4 x the restatement's own figure
    assert ref.K == 4 * ref.RESTATEMENT_BOUND and ref.K & (ref.K - 1) == 0
    assert max(worst["worst_dist"], worst["worst_weights"]) > ref.RESTATEMENT_BOUND / 2  # ... rounded UP to a power of two, not more
    assert worst["worst_sum_u"] == 0.0  # the weights sum to 1 exactly


def test_expanded_quadratic_fails_the_rule_near_the_surface(shapes):
    """d2 from |v|^2 - 2 s (e1.v) - ... instead of the residual vector: thousands of u R on the sources on the surface and at
    normal noise 1e-4, on the mesh at the origin and on the offset mesh."""
    for offset in ((0.0, 0.0, 0.0), (100.0, 100.0, 100.0)):
        B, N, T = ref.OFFSET_SHAPE
        c = ref.parity_case(B, N, T, False, offset=offset)
        near = np.arange(N) % 4 < 2
        src = np.ascontiguousarray(c["source"][:, near])
        face, bary, points, dist2 = ref.expanded32(src, c["vertices"], c["triangles"])
        with pytest.raises(AssertionError, match="dist2"):
            ref.check(src, c["vertices"], c["triangles"], face, None, None, dist2)
        d, R = ref.brute_force64(src, c["vertices"], c["triangles"])
        pick = lambda x: np.take_along_axis(x, face[..., None].astype(np.int64), -1)[..., 0]
        with np.errstate(invalid="ignore"):
            fig = np.abs(np.sqrt(np.maximum(dist2.astype(np.float64), 0.0)) - pick(d)) / (ref.U * pick(R))
        print("expanded32 dist2 figure (u R), offset", offset, float(fig.max()))
        assert fig.max() > 4 * ref.K
        face, bary, points, dist2 = ref.restatement32(src, c["vertices"], c["triangles"])
        ref.check(src, c["vertices"], c["triangles"], face, bary, points, dist2)  # the residual form on the same sources


def test_analytic_cases():
    """Two right triangles over the unit square, sharing the edge b-c of face 0; every value is exact in float32."""
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    src = np.array([[[0.25, 0.25, 0.5], [0.5, -1, 0], [-1, -1, 0], [1, 0, 0], [0.5, 0.5, 0], [0.75, 0.75, 2], [2, 2, 0]]], np.float32)
    face, bary, points, dist2 = ref.restatement32(src, vtx, tri)
    assert face[0].tolist() == [0, 0, 0, 0, 0, 1, 1]  # above an interior, beyond edge ab, beyond vertex a, ON vertex b, ON the shared edge, face 1
    want_bary = [[0.5, 0.25, 0.25], [0.5, 0.5, 0], [1, 0, 0], [0, 1, 0], [0, 0.5, 0.5], [0.25, 0.5, 0.25], [0, 1, 0]]
    want_pts = [[0.25, 0.25, 0], [0.5, 0, 0], [0, 0, 0], [1, 0, 0], [0.5, 0.5, 0], [0.75, 0.75, 0], [1, 1, 0]]
    assert bary[0].tolist() == want_bary and points[0].tolist() == want_pts
    assert dist2[0].tolist() == [0.25, 1.0, 2.0, 0.0, 0.0, 4.0, 2.0]
    ref.check(src, vtx, tri, face, bary, points, dist2)
    # a repeated vertex and a NaN vertex: never returned; only degenerate faces: -1 / zeros / +inf
    tri2 = np.array([[0, 0, 1], [0, 1, 2], [1, 3, 2]], np.int32)
    f2 = ref.restatement32(src, vtx, tri2)[0]
    assert f2[0].tolist() == [1, 1, 1, 1, 1, 2, 2]
    face, bary, points, dist2 = ref.restatement32(src, vtx, tri2[:1])
    assert (face == -1).all() and (bary == 0).all() and (points == 0).all() and (dist2 == np.inf).all()
    ref.check(src, vtx, tri2[:1], face, bary, points, dist2)
    vnan = vtx.copy()
    vnan[0, 1] = np.nan
    assert ref.restatement32(src, vnan, tri)[0][0].tolist() == [1] * 7


def test_max_dist_values_leave_no_source_undecided():
    B, N, T = ref.MAX_DIST_SHAPE
    c = ref.parity_case(B, N, T, False)
    values = list(ref.MAX_DIST_VALUES)
    y = ref.brute_force64(c["source"], c["vertices"], c["triangles"])
    for md in values + [np.inf]:
        face, bary, points, dist2 = ref.restatement32(c["source"], c["vertices"], c["triangles"], md)
        st = ref.check(c["source"], c["vertices"], c["triangles"], face, bary, points, dist2, max_dist=md, yardstick=y)
        assert st["undecided"] == 0, (md, st)
        if 0 < md < np.inf:
            assert 0 < st["valid"] < st["sources"], (md, st)  # a mix of valid and invalid sources
