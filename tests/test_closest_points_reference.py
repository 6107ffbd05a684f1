"""The yardstick of the closest-point tests checked on its own (no GPU): on every cloud the GPU parity test uses, the plain
float32 restatement of the difference form stays inside the acceptance rule of tests/closest_points_reference.py against the
float64 brute force, and no case has more than 1 % of its sources undecided (max_dist) or with a target in the normal band
that would change the answer.  On the offset cloud (coordinates 100 +- 0.05) the expanded form |s|^2 + |t|^2 - 2 s.t does NOT
stay inside the rule: the case discriminates between the two forms."""
import numpy as np
import pytest

from momentum_amd import build as mbuild
from momentum_amd import capi
from tests import closest_points_reference as ref


def _cases():
    mbuild.build()
    out = []
    for normals in (False, True):
        for B, N, M in ref.parity_shapes(capi.closest_points_plan, normals) + [ref.OFFSET_SHAPE]:
            for shared in (False, True):
                out.append((B, N, M, normals, shared))
    return out


def _kwargs(c, normals, max_dist=np.inf):
    return dict(max_dist=max_dist, source_normals=c["source_normals"], target_normals=c["target_normals"], min_normal_dot=ref.MIN_NORMAL_DOT if normals else 0.0)


def test_float32_restatement_stays_inside_the_rule_on_every_parity_case():
    worst = dict(worst_ratio_u=0.0, worst_dist2_u=0.0, differ=0)
    for B, N, M, normals, shared in _cases():
        kind = "offset" if (B, N, M) == ref.OFFSET_SHAPE else "unit"
        c = ref.cloud(kind, B, N, M, ref.shape_seed(B, N, M, normals, shared), shared, normals)
        kw = _kwargs(c, normals)
        index, dist2 = ref.restatement32(c["source"], c["target"], **kw)
        s = ref.check(c["source"], c["target"], index, dist2, None, **kw)
        assert s["undecided"] * 100 <= s["sources"] and s["band"] * 100 <= s["sources"], ((B, N, M, normals, shared), s)
        for k in worst:
            worst[k] = max(worst[k], s[k])
    print(worst)
    assert worst["worst_ratio_u"] <= 16 and worst["worst_dist2_u"] <= 8


@pytest.mark.parametrize("max_dist", [0.05, 0.3])
def test_max_dist_cases_have_few_undecided_sources(max_dist):
    c = ref.cloud("unit", 3, 300, 700, 77)
    index, dist2 = ref.restatement32(c["source"], c["target"], max_dist=max_dist)
    s = ref.check(c["source"], c["target"], index, dist2, None, max_dist=max_dist)
    assert s["undecided"] * 100 <= s["sources"], s
    assert 0 < (index >= 0).sum() < index.size  # a mix of near and far sources


def test_expanded_form_fails_the_rule_on_the_offset_cloud():
    B, N, M = ref.OFFSET_SHAPE
    c = ref.cloud("offset", B, N, M, ref.shape_seed(B, N, M, False, False))
    good, _ = ref.restatement32(c["source"], c["target"])
    bad, bad_d2 = ref.expanded32(c["source"], c["target"])
    d, _ = ref.brute_force64(c["source"], c["target"])
    exact = d.argmin(-1)
    print("difference form differs from the float64 argmin at", int((good != exact).sum()), "of", exact.size, "sources; expanded form at", int((bad != exact).sum()))
    assert (good == exact).sum() >= 0.99 * exact.size
    assert (bad != exact).sum() >= 0.5 * exact.size
    with pytest.raises(AssertionError):
        ref.check(c["source"], c["target"], bad, None, None)


def test_check_catches_wrong_answers():
    """The rule itself: a farther target, a missed target, an index where none is eligible, a wrong dist2 and a wrong point are
    all refused."""
    c = ref.cloud("unit", 2, 50, 40, 5)
    index, dist2 = ref.restatement32(c["source"], c["target"])
    pts = np.take_along_axis(c["target"], index[..., None].astype(np.int64).repeat(3, -1), 1)
    ref.check(c["source"], c["target"], index, dist2, pts)
    for spoil in ("index", "none", "dist2", "points"):
        i, d, p = index.copy(), dist2.copy(), pts.copy()
        if spoil == "index":
            i[1, 3] = (i[1, 3] + 1) % 40
        elif spoil == "none":
            i[0, 0], d[0, 0] = -1, np.inf
        elif spoil == "dist2":
            d[1, 7] *= np.float32(1 + 2e-6)
        else:
            p[0, 2, 1] = np.nextafter(p[0, 2, 1], np.float32(9))
        with pytest.raises(AssertionError):
            ref.check(c["source"], c["target"], i, d, p)
    i, d = ref.restatement32(c["source"], c["target"], max_dist=1e-4)
    assert (i == -1).all()
    i[0, 0] = 0
    with pytest.raises(AssertionError):
        ref.check(c["source"], c["target"], i, None, None, max_dist=1e-4)
