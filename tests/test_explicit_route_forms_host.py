"""The shapes of tests/test_gpu_explicit_route_forms.py, checked without a GPU: that the named n and M reach every form of
the explicit-Jacobian route's two dispatchers (as transcribed in tests/explicit_route_forms.py), and that every solve shape
is one a single-precision solve CAN be held to its bounds on -- a condition on the inputs, settled here with the oracle's
float run before any GPU result is looked at."""
import numpy as np
import pytest

from tests import explicit_route_forms as F


def test_the_named_shapes_follow_the_dispatchers():
    assert F.NE_SHAPES[:4] == (1, 3, 31, 32) and F.NE_SHAPES[-4:] == (305, 383, 384, 385)
    bands = [(33, 80), (81, 112), (113, 144), (145, 160), (161, 208), (209, 240), (241, 272), (273, 304)]
    for (lo, hi), tpw, n in zip(bands, F.MFMA_TPW, F.NE_SHAPES[4:12]):
        assert lo <= n <= hi and n % 16 != 0
        assert F.ne_form(lo, 3600) == F.ne_form(hi, 3600) == F.ne_form(n, 3600) == ("mfma", tpw, True, 1)
    assert F.ne_form(1272, 3600) == ("valu", 32) and F.ne_form(1273, 3600) == ("valu", 16)
    for name in F.FULL_SETS:
        M, ns = F.CONSTRAINT_SETS[name], F.SOLVE_SHAPES[name]
        assert len(ns) == 10 and ns[4:] == (320, 321, 512, 513, 640, 641)
        assert F.cholesky_step_lds_bytes(ns[0], M) <= F.LDS_64K < F.cholesky_step_lds_bytes(ns[1], M)
        assert F.cholesky_step_lds_bytes(ns[2], M) <= F.LDS_160K < F.cholesky_step_lds_bytes(ns[3], M)
        assert ns[1] == ns[0] + 1 and ns[3] == ns[2] + 1 and 190 <= ns[2] <= 198
    assert F.CONSTRAINT_SETS["M3597"] % 4 == 1 and F.CONSTRAINT_SETS["M3597"] % 32 == 13 and F.CONSTRAINT_SETS["M3597"] % 16 == 13
    M = F.CONSTRAINT_SETS["M3591"]  # the residue at which `kk + 3 < M` / `row + 3 < M` decide, on every tiled form
    assert M % 4 == 3 and M % 16 != 0 and M % 32 != 0
    assert [F.step_form(n, M) for n in F.SOLVE_SHAPES["M3591"]] == [("tiled", 2, 32, False), ("tiled", 2, 16, False), ("tiled", 8, 16, False), ("tiled", 8, 16, True)]
    assert F.step_form(1496, 3600)[2] == 16 and F.step_form(2048, 3600)[2] == 8  # (chunkRows = 8 from ~1900 on)


def test_the_named_shapes_cover_every_form():
    ne = {F.ne_form(n, F.CONSTRAINT_SETS[name]) for name, n in F.NE_CASES}
    for tpw in F.MFMA_TPW:  # every instantiation of normalEquationsMfmaKernel<TPW, kVec>
        for vec in (True, False):
            assert any(f[:3] == ("mfma", tpw, vec) for f in ne), (tpw, vec)
    for vec in (True, False):
        for passes in (1, 2):
            assert ("mfma", 48, vec, passes) in ne
    assert {f[3] for f in ne if f[0] == "mfma"} == {1, 2}
    for name, M in F.CONSTRAINT_SETS.items():  # normalEquationsKernel, 32 rows, on either side of the matrix-core kernel
        assert any(n < 32 and F.ne_form(n, M) == ("valu", 32) for n in F.NE_SHAPES)
        assert any(n > 384 and F.ne_form(n, M) == ("valu", 32) for n in F.NE_SHAPES)
    # (the VALU kernel's 16-row chunks, n > 1272, and the tiled step's chunkRows = 8, n >~ 1900, stay with the 1496- and
    # 2048-parameter solves of tests/test_gpu_many_parameters.py: a J of that width is not a few-seconds case)
    step = {(F.step_form(n, F.CONSTRAINT_SETS[name]), F.step_vec4(F.CONSTRAINT_SETS[name])) for name, n in F.SOLVE_CASES}
    for vec4 in (True, False):
        assert (("lds", False), vec4) in step and (("lds", True), vec4) in step
        for tiled in (("tiled", 2, 32, False), ("tiled", 2, 16, False), ("tiled", 8, 16, False), ("tiled", 8, 16, True)):
            assert (tiled, vec4) in step, (tiled, vec4)
    M = F.CONSTRAINT_SETS["M3597"]
    assert [F.step_form(n, M) for n in F.DEFERRED_SHAPES] == [("lds", True), ("tiled", 2, 32, False), ("tiled", 2, 16, False), ("tiled", 8, 16, True)]
    assert M % 16 != 0 and M % 32 != 0  # the ragged last chunk of the tiled refinement at either chunk size


def test_the_enabled_sets_are_real_indirections():
    for n in sorted(set(F.NE_SHAPES) | {n for ns in F.SOLVE_SHAPES.values() for n in ns}):
        for name in F.CONSTRAINT_SETS:
            idx = np.flatnonzero(F.solve_enabled(name, n) if n in F.SOLVE_SHAPES[name] else F.enabled_set(n))
            assert len(idx) == n
            assert n < 4 or not np.array_equal(idx, np.arange(idx[0], idx[0] + n))


def _float_reference_checks(name, n, rule):
    r64, r32 = F.oracle_solve(name, n, rule, "f64"), F.oracle_solve(name, n, rule, "f32")
    dist = F.theta_distance(r32["theta"], r64["theta"])
    h, href = r32["error_history"], r64["error_history"]
    with np.errstate(invalid="ignore", divide="ignore"):
        hist = np.nanmax(np.abs(h - href) / (1e-4 * np.abs(href) + 1e-7 * href[:, :1]))
    print(f"float oracle {name} n={n} {rule}: theta {dist.max():.3g} history {hist:.3g} of its bound; iterations {r64['iterations']}")
    assert np.array_equal(r32["iterations"], r64["iterations"]) and np.array_equal(r32["status"], r64["status"])
    assert np.all(r64["status"] == 0)
    # element 1 stops at the first convergence test it is allowed and sits out the rest, the others take every iteration
    last = F.solve_options(rule).max_iterations
    assert r64["iterations"].tolist() == [last, 2, last]
    assert np.all(F.history_within_bound(h, href)), hist
    assert dist.max() <= 1e-5, dist  # (the GPU test's bound is max(1e-5, 3 x sensitivity): the float oracle needs no more than 1e-5)
    if rule == "lm_schedule":
        # the same accept / reject and damping decisions in float and double, for the elements that move (element 1 proposes
        # steps of rounding size from its solution: taken or not, its parameters stay where they are)
        for key in ("lambda_history", "gain_ratio_history"):
            assert r32[key].shape == r64[key].shape == (F.B, last)
        assert np.array_equal(r32["lambda_history"][[0, 2]], r64["lambda_history"][[0, 2]])
        assert np.array_equal(r32["gain_ratio_history"][[0, 2]] > 0, r64["gain_ratio_history"][[0, 2]] > 0)
        assert F.theta_distance(r32["theta"][1:2], F.solve_start(name, n)[1:2]).max() <= 1e-6
    return dist.max(), hist


@pytest.mark.parametrize("name,n", F.SOLVE_CASES, ids=[f"{name}-n{n}" for name, n in F.SOLVE_CASES])
def test_the_float_reference_stays_inside_the_solve_bound(name, n):
    """If a shape fails here, change its seed (SOLVE_SALT) in tests/explicit_route_forms.py -- never the bound."""
    _float_reference_checks(name, n, "plain")


@pytest.mark.parametrize("n,rule", F.DEFERRED_CASES, ids=[f"n{n}-{rule}" for n, rule in F.DEFERRED_CASES])
def test_the_float_reference_stays_inside_the_deferred_step_bound(n, rule):
    _float_reference_checks("M3597", n, rule)
