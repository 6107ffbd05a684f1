"""Reference and acceptance rule of mmx_closest_points (include/mmx.h), shared by the host tests and the GPU tests.

brute_force64    numpy brute force in float64 on the float32 inputs: the distances d64 [B, N, M] and, with normals, the
                 dots.  The yardstick of every check.
restatement32    the difference form in plain float32 numpy: dx = s.x - t.x ... first, d2 = dx*dx + dy*dy + dz*dz, the first
                 minimum among the eligible targets.  What the kernel states, without its fma.
expanded32       the form a caller gets from cdist: |s|^2 + |t|^2 - 2 s.t in float32.  NOT what the kernel does; it is here
                 to show that the offset cloud discriminates.
check            the acceptance rule.  With u = 2^-24: each float32 difference has relative error <= u, each square adds u,
                 the two additions u each, so a computed d2 is within about 5u of the true value (the restatement measures at
                 most 4.7u), and a choice j made on computed values satisfies d64(j) <= (1 + 16u) min d64: 10u for two such
                 errors plus slack for fma contraction.  dist2 must be within 8u of d64(index).  max_dist: valid must be
                 true when min d64 <= maxd^2 (1 - 16u), false when min d64 > maxd^2 (1 + 16u), either in between
                 ("undecided").  Normals, with d = 1e-6: the chosen target has dot >= min_normal_dot - d, its distance is
                 within (1 + 16u) of the minimum over targets with dot >= min_normal_dot + d, and the result is -1 when no
                 target reaches min_normal_dot - d.  check() returns the counts of undecided sources and of sources with a
                 target in the normal band nearer than every surely eligible one; the host test caps both at 1 % per case.
cases            the seeded clouds and the shape list of the parity tests, taken from mmx_closest_points_plan.
"""
import numpy as np

U = 2.0**-24
DOT_BAND = 1e-6
INDEX_SLACK = 16 * U
DIST2_SLACK = 8 * U


def _bcast_target(target, B):
    target = np.asarray(target)
    return np.broadcast_to(target, (B,) + target.shape) if target.ndim == 2 else target


def brute_force64(source, target, source_normals=None, target_normals=None):
    """(d64 [B, N, M], dot64 [B, N, M] or None) in float64 on the float32 inputs; target may be [M, 3] (shared)."""
    s = np.asarray(source, np.float32).astype(np.float64)
    B = s.shape[0]
    t = _bcast_target(np.asarray(target, np.float32), B).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.zeros((B, s.shape[1], t.shape[1]))
        for c in range(3):
            d += (s[:, :, None, c] - t[:, None, :, c]) ** 2
        dot = None
        if source_normals is not None:
            ns = np.asarray(source_normals, np.float32).astype(np.float64)
            nt = _bcast_target(np.asarray(target_normals, np.float32), B).astype(np.float64)
            dot = np.einsum("bnc,bmc->bnm", ns, nt)
    return d, dot


def _pick32(d2, eligible, max_dist):
    """first minimum of the float32 d2 [B, N, M] over the eligible targets -> (index int32, dist2 float32)"""
    with np.errstate(invalid="ignore", over="ignore"):
        m2 = np.float32(max_dist) * np.float32(max_dist)
        ok = eligible & np.isfinite(d2) & (d2 <= m2)
    masked = np.where(ok, d2, np.float32(np.inf))
    idx = masked.argmin(-1).astype(np.int32)
    best = np.take_along_axis(masked, idx[..., None].astype(np.int64), -1)[..., 0]
    none = ~ok.any(-1)
    return np.where(none, np.int32(-1), idx), np.where(none, np.float32(np.inf), best).astype(np.float32)


def _eligible32(B, source_normals, target_normals, min_normal_dot, shape):
    if source_normals is None:
        return np.ones(shape, bool)
    ns = np.asarray(source_normals, np.float32)
    nt = _bcast_target(np.asarray(target_normals, np.float32), B)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = ns[:, :, None, 0] * nt[:, None, :, 0]
        dot = dot + ns[:, :, None, 1] * nt[:, None, :, 1]
        dot = dot + ns[:, :, None, 2] * nt[:, None, :, 2]
        return dot >= np.float32(min_normal_dot)


def restatement32(source, target, max_dist=np.inf, source_normals=None, target_normals=None, min_normal_dot=0.0):
    """The difference form in float32: (index [B, N] int32, dist2 [B, N] float32)."""
    s = np.asarray(source, np.float32)
    t = _bcast_target(np.asarray(target, np.float32), s.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (s[:, :, None, c] - t[:, None, :, c] for c in range(3))
        d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == np.float32
    return _pick32(d2, _eligible32(s.shape[0], source_normals, target_normals, min_normal_dot, d2.shape), max_dist)


def expanded32(source, target, max_dist=np.inf, source_normals=None, target_normals=None, min_normal_dot=0.0):
    """|s|^2 + |t|^2 - 2 s.t in float32 (what cdist-style code computes): (index, dist2)."""
    s = np.asarray(source, np.float32)
    t = _bcast_target(np.asarray(target, np.float32), s.shape[0])
    d2 = (s * s).sum(-1)[:, :, None] + (t * t).sum(-1)[:, None, :] - np.float32(2) * np.einsum("bnc,bmc->bnm", s, t)
    assert d2.dtype == np.float32
    return _pick32(d2, _eligible32(s.shape[0], source_normals, target_normals, min_normal_dot, d2.shape), max_dist)


def check(source, target, index, dist2=None, points=None, max_dist=np.inf, source_normals=None, target_normals=None, min_normal_dot=0.0):
    """Asserts the acceptance rule (module docstring) on a result and returns its figures:
    dict(sources, worst_ratio_u, worst_dist2_u, differ, undecided, band)."""
    index = np.asarray(index)
    B, N = index.shape
    d, dot = brute_force64(source, target, source_normals, target_normals)
    fin = np.isfinite(d)
    if dot is None:
        lo = hi = fin
    else:
        with np.errstate(invalid="ignore"):
            lo, hi = fin & (dot >= min_normal_dot - DOT_BAND), fin & (dot >= min_normal_dot + DOT_BAND)
    min_lo, min_hi = np.where(lo, d, np.inf).min(-1), np.where(hi, d, np.inf).min(-1)
    m2 = float(np.float32(max_dist)) ** 2
    must_valid = np.isfinite(min_hi) & (min_hi <= m2 * (1 - INDEX_SLACK))
    must_invalid = ~(np.isfinite(min_lo) & (min_lo <= m2 * (1 + INDEX_SLACK)))
    undecided = ~must_valid & ~must_invalid
    band = ~must_invalid & (min_lo * (1 + INDEX_SLACK) < min_hi)
    got = index >= 0
    assert index.dtype == np.int32 and (index >= -1).all() and (index < d.shape[2]).all()
    assert not (must_valid & ~got).any(), f"{(must_valid & ~got).sum()} sources have a surely eligible target and got -1"
    assert not (must_invalid & got).any(), f"{(must_invalid & got).sum()} sources have no eligible target and got an index"
    j = np.where(got, index, 0).astype(np.int64)[..., None]
    dj = np.take_along_axis(d, j, -1)[..., 0]
    assert np.take_along_axis(lo, j, -1)[..., 0][got].all(), "a chosen target is not finite or fails the normal test by more than the band"
    assert (dj[got] <= m2 * (1 + INDEX_SLACK)).all(), "a chosen target is beyond max_dist"
    assert (dj[got] <= (1 + INDEX_SLACK) * min_hi[got]).all(), "a chosen target is farther than (1 + 16u) x the nearest eligible one"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(got & np.isfinite(min_hi) & (min_hi > 0), dj / min_hi - 1, 0.0)
    stats = dict(sources=int(B * N), worst_ratio_u=float(ratio.max() / U), worst_dist2_u=0.0, undecided=int(undecided.sum()), band=int(band.sum()))
    stats["differ"] = int((got & (index != np.where(hi, d, np.inf).argmin(-1))).sum())
    if dist2 is not None:
        dist2 = np.asarray(dist2)
        assert dist2.dtype == np.float32 and (dist2[~got] == np.inf).all(), "dist2 must be +inf where index is -1"
        err = np.abs(dist2[got].astype(np.float64) - dj[got])
        assert (err <= DIST2_SLACK * dj[got]).all(), "dist2 is farther than 8u from d64(index)"
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(dj[got] > 0, err / dj[got], 0.0)
        stats["worst_dist2_u"] = float(rel.max() / U) if rel.size else 0.0
    if points is not None:
        points = np.asarray(points)
        t = _bcast_target(np.asarray(target, np.float32), B)
        want = np.where(got[..., None], t[np.arange(B)[:, None], j[..., 0]], np.float32(0))
        assert points.dtype == np.float32 and points.shape == (B, N, 3)
        assert (points.view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).all(), "points is not a copy of the chosen target (zeros where -1)"
    return stats


# ---- the seeded clouds and the parity shape list
def unit_normals(rng, shape):
    n = rng.standard_normal(shape + (3,))
    return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)


def cloud(kind, B, N, M, seed, shared=False, normals=False):
    """dict(source [B,N,3], target [B,M,3] or [M,3], source_normals, target_normals (or None)), float32, seeded.
    kind "unit": uniform in [-1, 1]^3; "offset": coordinates 100 +- 0.05."""
    rng = np.random.default_rng(seed)
    mid, half = (100.0, 0.05) if kind == "offset" else (0.0, 1.0)
    tshape = (M,) if shared else (B, M)
    c = dict(source=(mid + half * rng.uniform(-1, 1, (B, N, 3))).astype(np.float32), target=(mid + half * rng.uniform(-1, 1, tshape + (3,))).astype(np.float32))
    c["source_normals"] = unit_normals(rng, (B, N)) if normals else None
    c["target_normals"] = unit_normals(rng, tshape) if normals else None
    return c


MIN_NORMAL_DOT = 0.25  # the parity cases with normals
OFFSET_SHAPE = (2, 200, 2000)  # the offset cloud's (B, N, M)


def parity_shapes(plan, normals):
    """The (B, N, M) list of the parity tests for one kernel instantiation, from plan = capi.closest_points_plan (S sources per
    workgroup, T targets per tile, W ways): the four fixed shapes, N in {S-1, S, S+1}, M in {T-1, T, T+1, 2T+1} and, when W > 1,
    M in {W-1, W+1}."""
    shapes = [(1, 1, 1), (3, 63, 65), (2, 64, 64), (2, 65, 1)]
    p = plan(2, 64, 64, normals)
    S, T, W = p["sources_per_workgroup"], p["target_tile"], p["target_ways"]
    shapes += [(2, n, 65) for n in (S - 1, S, S + 1)] + [(2, 2, m) for m in (T - 1, T, T + 1, 2 * T + 1)]
    if W > 1:
        shapes += [(2, 65, m) for m in (W - 1, W + 1)]
    return shapes


def shape_seed(B, N, M, normals, shared):
    return 1000003 * B + 1009 * N + 7 * M + 2 * int(normals) + int(shared)
