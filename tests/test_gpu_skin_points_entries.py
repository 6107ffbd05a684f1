"""mmx_skin_points / mmx_skin_points_backward on the GPU entry by entry: every entry of out, rest_grad and state_grad against
the float64 reference under the per-entry rules of tests/skinning_reference.py (entry_bounds; shown sound and with teeth on the
CPU in tests/test_skinning_reference.py), where tests/test_gpu_skin_points.py takes the max-norm of an instance:

    out, rest_grad    |x - x64| <= (K + 7) u A                         u = 2^-24, A the sum of the absolute terms of the entry
    state_grad        |x - x64| <= u |x64| + (n_j + 64) 2^-52 S        n_j the joint's entry count, S the twelve-sum formulas
                                                                       on absolute values; S = 0 asks for a zero

on states no forward kinematics gives (arbitrary_states: non-unit and zero quaternions, negative, tiny and zero scales,
translations of size 10), on entry lists pinned at the edges of the backward loop (1, 63/64/65, 255/256/257, 511/512/513
entries, empty joints inside packed waves, 1 .. 7 waves), at the 255 / 258-row edge of the posed-affine build, with every output
placed between guard rows, and with -0.0 padding.

Measured on an MI355X (worst entry over the instances; profiles/skin_points_entry_bounds.json, written through MMX_PARITY_OUT
by a run of this file alone).  out / rest_grad: err / (u A), allowed K + 7; state_grad: (err - u |x64|) / ((n_j + 64) 2^-52 S),
allowed 1 -- negative where every entry is within one float32 rounding of the float64 value, and then the largest
err / (u |x64|) says how much of that rounding is used (the figures are over the entries with S > 0; the others are zeros):
    character3_k4_b5/arbitrary/shared_rest   out 1.29 of 11   rest_grad 1.74 of 11   state_grad -2.34e+04 (err / (u |x64|) 0.901)
    character3_k4_b5/arbitrary/instance_rest out 1.46 of 11   rest_grad 1.74 of 11   state_grad -9.51e+03 (err / (u |x64|) 0.845)
    k8/arbitrary/shared_rest                 out 1.84 of 15   rest_grad 2.76 of 15   state_grad -65       (err / (u |x64|) 0.943)
    k8/arbitrary/instance_rest               out 1.85 of 15   rest_grad 2.76 of 15   state_grad -3.23     (err / (u |x64|) 0.965)
    humanoid72/arbitrary/shared_rest         out 2.30 of 11   rest_grad 3.11 of 11   state_grad -0.664    (err / (u |x64|) 0.965)
    humanoid72/arbitrary/instance_rest       out 3.38 of 11   rest_grad 3.11 of 11   state_grad -1.55     (err / (u |x64|) 0.975)
    wild_weights/arbitrary/shared_rest       out 1.79 of 15   rest_grad 2.46 of 15   state_grad -3.44     (err / (u |x64|) 0.867)
    wild_weights/arbitrary/instance_rest     out 2.07 of 15   rest_grad 2.46 of 15   state_grad -56.3     (err / (u |x64|) 0.970)
    character3_k4_b5/fk/shared_rest          out 2.02 of 11   rest_grad 1.47 of 11   state_grad -2.61e+03 (err / (u |x64|) 0.902)
    k8/fk/shared_rest                        out 1.64 of 15   rest_grad 2.33 of 15   state_grad -1.93     (err / (u |x64|) 0.980)
    humanoid72/fk/shared_rest                out 2.02 of 11   rest_grad 2.51 of 11   state_grad -0.568    (err / (u |x64|) 0.954)
    wild_weights/fk/shared_rest              out 1.21 of 15   rest_grad 2.31 of 15   state_grad -4.73     (err / (u |x64|) 0.883)
    list_lengths                             out 2.24 of 8    rest_grad 2.79 of 8    state_grad -189      (err / (u |x64|) 0.907)
    list_lengths/instance_rest               out 2.32 of 8    rest_grad 2.79 of 8    state_grad -90.3     (err / (u |x64|) 0.925)
    equal_lists_j1                           out 1.79 of 8    rest_grad 2.23 of 8    state_grad -3.74e+04 (err / (u |x64|) 0.657)
    equal_lists_j2                           out 2.20 of 8    rest_grad 2.12 of 8    state_grad -7.32e+03 (err / (u |x64|) 0.913)
    equal_lists_j3                           out 1.89 of 8    rest_grad 2.32 of 8    state_grad -4.56e+03 (err / (u |x64|) 0.867)
    equal_lists_j5                           out 2.19 of 8    rest_grad 2.34 of 8    state_grad -1.12e+03 (err / (u |x64|) 0.859)
    equal_lists_j6                           out 2.42 of 8    rest_grad 2.82 of 8    state_grad -75.1     (err / (u |x64|) 0.939)
    equal_lists_j7                           out 2.33 of 8    rest_grad 2.47 of 8    state_grad -1.00e+03 (err / (u |x64|) 0.880)
    affine_rows_j85                          out 2.40 of 9    rest_grad 3.33 of 9    state_grad -784      (err / (u |x64|) 0.956)
    affine_rows_j86                          out 2.38 of 9    rest_grad 2.80 of 9    state_grad -63.1     (err / (u |x64|) 0.959)
    negative_zero_padding                    out 1.83 of 11   rest_grad 1.74 of 11   state_grad -1.66e+04 (err / (u |x64|) 0.890)
Every entry holds its rule: vertices and rest gradient use 1.2 to 3.4 of the K + 7 roundings allowed (the float32 restatement
of the kernel's order in tests/test_skinning_reference.py uses 1.4 to 2.8 on its four cases), and no entry of the state gradient is further from the float64 value than
one float32 rounding of it (0.66 to 0.98 u), on arbitrary states as on forward-kinematics ones.
"""
import json
import os

import numpy as np
import pytest
import torch

from momentum_amd import capi, make_test_character, make_test_skin
from tests import skeleton_state_reference as fk
from tests import skinning_reference as ref
from tests.test_gpu_skin_points import SHAPES, Case, _cot, _cuda, _run_gpu, _run_ref

pytestmark = pytest.mark.gpu
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _write_worst():
    """MMX_PARITY_OUT=<file>: the worst ratios of this run as JSON (how profiles/skin_points_entry_bounds.json is made)."""
    yield
    out = os.environ.get("MMX_PARITY_OUT")
    if out and _worst:
        unit = ("worst entry over the instances.  out / rest_grad: err_over_uA = |x - x64| / (u A), allowed = K + 7; state_grad: "
                "ratio = (|x - x64| - u |x64|) / ((n_j + 64) 2^-52 S), allowed = 1; u = 2^-24")  # fmt: skip
        with open(out, "w") as f:
            json.dump(dict(unit=unit, shapes=_worst), f, indent=1)


def _used(case):
    return np.unique(case.joint[case.weight != 0])


def _assert_rules(name, case, state, cot, rest=None, got=None):
    """The three rules on every entry; returns the GPU's outputs."""
    got = _run_gpu(case, state, cot, rest) if got is None else got
    want = _run_ref(case, state, cot, torch.float64, rest)
    bounds = ref.entry_bounds(case.joint, case.weight, case.inv, case.rest if rest is None else rest, state, cot)
    over = {}
    for key in ("out", "rest_grad", "state_grad"):
        r = ref.entry_ratios(key, got[key], want[key], bounds, case.K)
        if key == "state_grad":  # (the figures: over the entries with S > 0; the others must be zeros, asserted below)
            live = (bounds["state_grad"] > 0) & (want[key] != 0)
            roundings = np.abs(got[key].astype(np.float64) - want[key])[live] / (ref.U32 * np.abs(want[key][live]))
            _worst[f"{name}/{key}"] = dict(ratio=float(r[live].max()), allowed=1.0, err_over_u_ref=float(roundings.max()))
            print(f"{name}/{key}: worst (err - u|ref|) / ((n + 64) 2^-52 S) {r[live].max():.3g}, worst err / (u |ref|) {roundings.max():.3g}")
        else:
            _worst[f"{name}/{key}"] = dict(err_over_uA=float(r.max() * (case.K + 7)), allowed=float(case.K + 7))
            print(f"{name}/{key}: worst err / (u A) {r.max() * (case.K + 7):.3g} of {case.K + 7}")
        over[key] = r
    for key, r in over.items():
        assert np.isfinite(got[key]).all(), (name, key)
        at = np.unravel_index(np.argmax(r), r.shape)
        assert r.max() <= 1.0, (name, key, at, float(r.max()), got[key][at], want[key][at])
    # a joint without entries: eight exact zeros; S = 0 elsewhere (scale 0, the zero quaternion): a zero of either sign
    n, S = bounds["entries"], bounds["state_grad"]
    assert np.all(got["state_grad"][:, n == 0] == 0.0) and not np.signbit(got["state_grad"][:, n == 0]).any()
    assert np.all(got["state_grad"][S == 0] == 0.0)
    return got


def _instance_rest(case, B, seed):
    return (case.rest[None] + 0.05 * np.random.default_rng(seed).normal(size=(B, case.V, 3))).astype(np.float32)


def _wild():
    """Weights uniform in [-1, 1.5], not normalised, a quarter of them zero; vertex 7 names joint 4 in two slots."""
    rig = fk.all_dofs_rig(fk.random_tree(7, seed=3), seed=3)
    s = make_test_skin(rig, 200, 8, 44, random_affine=True)
    rng = np.random.default_rng(45)
    joint = rng.integers(0, 7, size=(200, 8)).astype(np.int32)
    weight = rng.uniform(-1.0, 1.5, size=(200, 8)).astype(np.float32)
    weight[rng.uniform(size=(200, 8)) < 0.25] = 0.0
    joint[7, 2], joint[7, 5] = 4, 4
    weight[7, 2], weight[7, 5] = 0.75, -0.5
    return Case(rig, joint, weight, s.inverse_bind, s.rest)


def _star(J, seed):
    return fk.all_dofs_rig([-1] + [0] * (J - 1), seed=seed)


def _list_case(counts, seed):
    """K = 1 on a star rig: counts[j] vertices on joint j, the vertex order shuffled; a full random 3 x 4 inverse bind."""
    rng = np.random.default_rng(seed)
    J = len(counts)
    joint = rng.permutation(np.repeat(np.arange(J), counts)).astype(np.int32)[:, None]
    V = joint.shape[0]
    weight = rng.uniform(0.25, 1.0, size=(V, 1)).astype(np.float32)
    case = Case(_star(J, seed), joint, weight, rng.normal(size=(J, 12)).astype(np.float32), rng.normal(size=(V, 3)).astype(np.float32))
    assert np.array_equal(np.diff(capi.host_skin_tables(J, joint, weight)["joint_start"]), counts)
    return case


def _random_case(rig, V, K, seed):
    """Every slot a random joint with a positive weight (rows sum to 1); the last joint is named by vertex 0."""
    rng = np.random.default_rng(seed)
    J = rig.num_joints
    joint = rng.integers(0, J, size=(V, K)).astype(np.int32)
    joint[0, 0] = J - 1
    weight = rng.uniform(0.1, 1.0, size=(V, K))
    weight = (weight / weight.sum(1, keepdims=True)).astype(np.float32)
    return Case(rig, joint, weight, rng.normal(size=(J, 12)).astype(np.float32), rng.normal(size=(V, 3)).astype(np.float32))


CASES = {
    "character3_k4_b5": SHAPES["character3_k4_b5"],
    "k8": SHAPES["k8"],
    "humanoid72": SHAPES["humanoid72"],
    "wild_weights": (_wild, 3),
}
# the list-length skin: 8 waves, waveStart = [0, 6, 7, 8, 11, 12, 13, 14, 16] (tests/cpp/test_skin_tables.cpp): wave 0 packs the
# joints 0 .. 5 and wave 3 the joints 8 .. 10, empty ones included
LIST_COUNTS = [0, 1, 63, 64, 65, 0, 255, 256, 257, 0, 0, 511, 512, 513, 0, 0]


@pytest.mark.parametrize("rest_kind", ["shared_rest", "instance_rest"])
@pytest.mark.parametrize("name", list(CASES))
def test_arbitrary_states_entry_by_entry(torch_cuda, name, rest_kind):
    mk, B = CASES[name]
    case = mk()
    state = ref.arbitrary_states(case.J, B, seed=1100 + len(name), used=_used(case))
    cot = _cot(case, B, 1200 + len(name))
    rest = _instance_rest(case, B, 1300) if rest_kind == "instance_rest" else None
    got = _assert_rules(f"{name}/arbitrary/{rest_kind}", case, state, cot, rest)
    used = _used(case)
    # the planted rows are there, on joints that have entries, and the states are nothing forward kinematics gives
    on = state[:, used]
    assert (np.abs(on[..., 3:7]).max(-1) == 0).any() and (on[..., 7] == 0).any() and (on[..., 7] < 0).any()
    assert np.all(np.abs(got["state_grad"][:, used, :3]).max(axis=2) > 0.0)
    if name == "wild_weights":
        assert (case.weight < 0).any() and (case.weight == 0).mean() > 0.2 and case.joint[7, 2] == case.joint[7, 5]


@pytest.mark.parametrize("name", ["character3_k4_b5", "k8", "humanoid72", "wild_weights"])
def test_forward_kinematics_states_entry_by_entry(torch_cuda, name):
    mk, B = CASES[name]
    case = mk()
    _assert_rules(f"{name}/fk/shared_rest", case, case.states(B, seed=1400 + len(name)), _cot(case, B, 1500 + len(name)))


def test_entry_lists_at_the_edges_of_the_backward_loop(torch_cuda):
    case = _list_case(LIST_COUNTS, seed=21)
    assert case.V == 2497 and case.J == 16
    B = 3
    empty = np.array([j for j, c in enumerate(LIST_COUNTS) if c == 0])
    state, cot = ref.arbitrary_states(case.J, B, seed=22, used=_used(case)), _cot(case, B, 23)
    got = _assert_rules("list_lengths", case, state, cot)
    # NaN in the state rows of the joints without entries: their rows are exact +0, everything else has the same bits
    bad = state.copy()
    bad[:, empty] = np.nan
    got_bad = _run_gpu(case, bad, cot)
    for g in (got, got_bad):
        assert np.all(g["state_grad"][:, empty] == 0.0) and not np.signbit(g["state_grad"][:, empty]).any()
    for key in got:
        assert np.array_equal(got[key].view(np.uint32), got_bad[key].view(np.uint32)), key
    rest = _instance_rest(case, B, 24)
    _assert_rules("list_lengths/instance_rest", case, state, cot, rest)


@pytest.mark.parametrize("J", [1, 2, 3, 5, 6, 7])
def test_equal_lists_give_every_count_of_live_waves(torch_cuda, J):
    """40 entries on each of J joints: a wave per joint (tests/cpp/test_skin_tables.cpp), so J waves -- every residue modulo
    the four waves of a workgroup, a last workgroup with one, two and three live waves."""
    case = _list_case([40] * J, seed=30 + J)
    B = 3
    _assert_rules(f"equal_lists_j{J}", case, ref.arbitrary_states(J, B, seed=40 + J), _cot(case, B, 50 + J))


@pytest.mark.parametrize("J", [85, 86])
def test_posed_affine_build_at_255_and_258_rows(torch_cuda, J):
    """3 J rows, one per thread of 256: 255 rows leave a thread idle, 258 send two threads round again."""
    case = _random_case(_star(J, seed=60), 300, 2, 61 + J)
    B = 2
    assert len(_used(case)) > 80 and J - 1 in _used(case)
    _assert_rules(f"affine_rows_j{J}", case, ref.arbitrary_states(J, B, seed=62 + J, used=_used(case)), _cot(case, B, 63 + J))


def _assert_every_write_and_nothing_else(case, state, cot, rest=None):
    """The three outputs as rows 1 .. B of tensors of B + 2 rows: the inside prefilled with NaN, the guard rows with -7.25."""
    B = state.shape[0]
    st, g = _cuda(state), _cuda(cot)
    r = None if rest is None else _cuda(rest)
    full = {key: torch.full((B + 2,) + shape, -7.25, device="cuda") for key, shape in (("out", (case.V, 3)), ("state_grad", (case.J, 8)), ("rest_grad", (case.V, 3)))}
    inside = {}
    for key, t in full.items():
        t[1 : B + 1] = float("nan")
        inside[key] = t[1 : B + 1]
        assert inside[key].is_contiguous() and inside[key].data_ptr() != t.data_ptr()
    case.skin.skin_points(st, r, out=inside["out"])
    case.skin.skin_points_backward(st, g, r, state_grad=inside["state_grad"], rest_grad=inside["rest_grad"])
    torch.cuda.synchronize()
    plain = _run_gpu(case, state, cot, rest)
    for key, t in full.items():
        a = t.cpu().numpy()
        assert np.isfinite(a[1 : B + 1]).all(), key  # every entry written
        guard = np.full(a[0].shape, -7.25, np.float32).view(np.uint32)
        assert np.array_equal(a[0].view(np.uint32), guard) and np.array_equal(a[B + 1].view(np.uint32), guard), key  # nothing else
        assert np.array_equal(a[1 : B + 1].view(np.uint32), plain[key].view(np.uint32)), key


@pytest.mark.parametrize("rest_kind", ["shared_rest", "instance_rest"])
@pytest.mark.parametrize("V", [1, 63, 1023, 1024, 1025])
def test_every_entry_is_written_and_nothing_else(torch_cuda, V, rest_kind):
    case = Case.synthetic(make_test_character(3), V, 2, 70 + V)
    B = 2
    state, cot = ref.arbitrary_states(case.J, B, seed=71 + V, used=_used(case)), _cot(case, B, 72 + V)
    _assert_every_write_and_nothing_else(case, state, cot, _instance_rest(case, B, 73) if rest_kind == "instance_rest" else None)


@pytest.mark.parametrize("name", ["list_lengths", "affine_rows_j85", "affine_rows_j86"])
def test_every_entry_is_written_and_nothing_else_on_the_edge_skins(torch_cuda, name):
    if name == "list_lengths":
        case, B = _list_case(LIST_COUNTS, seed=21), 3
    else:
        J = int(name[-2:])
        case, B = _random_case(_star(J, seed=60), 300, 2, 61 + J), 2
    _assert_every_write_and_nothing_else(case, ref.arbitrary_states(case.J, B, seed=81, used=_used(case)), _cot(case, B, 82))


def test_negative_zero_weight_is_padding_on_the_gpu(torch_cuda):
    """A slot of weight -0.0 (and one of +0.0) names joint 2, whose state row is NaN or inf: all three outputs have the bits
    of the run with a finite row."""
    joint, weight, rest = ref.hand_skin("character3_k4")
    weight = weight.copy()
    minus = (joint == 2) & (weight == 0)
    minus[2, 3] = False  # (one slot on joint 2 stays +0.0)
    weight[minus] = -0.0
    assert np.signbit(weight[minus]).all() and minus.sum() >= 4 and ((joint == 2) & (weight == 0) & ~np.signbit(weight)).sum() == 1
    rig = make_test_character(3)
    case = Case(rig, joint, weight, make_test_skin(rig, 1, 1, 0).inverse_bind, rest)
    B = 3
    state, cot = ref.arbitrary_states(case.J, B, seed=91, used=[0, 1]), _cot(case, B, 92)
    base = _assert_rules("negative_zero_padding", case, state, cot)
    bad = state.copy()
    bad[:, 2] = np.nan
    bad[1, 2] = -np.inf
    got = _run_gpu(case, bad, cot)
    for key in base:
        assert np.isfinite(got[key]).all() and np.array_equal(got[key].view(np.uint32), base[key].view(np.uint32)), key
    assert np.all(got["state_grad"][:, 2] == 0.0) and not np.signbit(got["state_grad"][:, 2]).any()
