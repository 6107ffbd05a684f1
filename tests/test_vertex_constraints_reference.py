"""The reference of mmx_skin_normal_equations' tests, checked on the CPU before anything is measured against it
(tests/vertex_constraints_reference.py): its float64 Jacobian agrees with central finite differences and, row by row, with the
composition of the two numpy restatements that already have their own checks -- skinning_reference.vjp_np (the twelve sums per
joint) followed by skeleton_state_reference.vjp_np (the channel formulas): row r of J is
skeleton_state_backward(skin_points_backward(cotangent of row r)).  Also: the skip rules, the enabled compaction, and that the
two-sum form the kernel takes per column source (m0 = sum coef, m1 = sum coef y over the influences under the source's joint)
gives the same rows.
"""
import numpy as np
import pytest
import torch

from momentum_amd import make_test_character, make_test_skin
from tests import skeleton_state_reference as fk
from tests import skinning_reference as skr
from tests import vertex_constraints_reference as vcr


def _character3():
    rig = make_test_character(3)
    joint, weight, rest = skr.hand_skin("character3_k4")
    return rig, (joint, weight, make_test_skin(rig, 1, 1, 0).inverse_bind, rest)


def _random_tree():
    # every dof of every joint (scales included), non-zero pt_offsets
    rig = fk.all_dofs_rig(fk.random_tree(9, 3), seed=4)
    rig.pt_offsets = np.random.default_rng(5).uniform(-0.2, 0.2, size=7 * rig.num_joints).astype(np.float32)
    s = make_test_skin(rig, 12, 3, 6, True)
    return rig, (s.joint, s.weight, s.inverse_bind, s.rest)


def _table():
    # parameters that drive several joints, a parameter that drives nothing, non-zero pt_offsets
    rig = fk.table_rig()
    s = make_test_skin(rig, 8, 2, 7, True)
    return rig, (s.joint, s.weight, s.inverse_bind, s.rest)


RIGS = {"character3": _character3, "random_tree": _random_tree, "table": _table}


def _constraints(V, B, C, S, plane, seed):
    rng = np.random.default_rng(seed)
    vertex = rng.integers(0, V, size=(B, C, S)).astype(np.int32)
    bary = rng.dirichlet(np.ones(3), size=(B, C)).astype(np.float32) if S == 3 else None
    normal = rng.normal(size=(B, C, 3)).astype(np.float32) if plane else None
    return vcr.Constraints(
        rng.normal(size=(B, C, 3)).astype(np.float32), vertex, bary, normal, rng.uniform(0.5, 2.0, size=(B, C)).astype(np.float32), 0.7
    )


CASES = [(name, S, plane) for name in RIGS for S in (1, 3) for plane in (False, True)]


@pytest.mark.parametrize("name,S,plane", CASES)
def test_jacobian_against_finite_differences(name, S, plane):
    rig, skin = RIGS[name]()
    B = 2
    theta, _ = fk.random_inputs(rig, B, 11)
    con = _constraints(len(skin[0]), B, 5, S, plane, 12)
    rt, sk = fk.RigTensors(rig), skr.SkinTensors(*skin, rig.num_joints)
    _, J = vcr.jacobian(rt, sk, theta, con)
    h = 1e-6
    th = torch.as_tensor(theta.astype(np.float64))
    fd = np.zeros_like(J)
    for p in range(rig.num_params):
        e = torch.zeros_like(th)
        e[:, p] = h
        fd[:, :, p] = ((vcr.scaled_rows(rt, sk, th + e, con) - vcr.scaled_rows(rt, sk, th - e, con)) / (2 * h)).numpy()
    assert np.abs(J).max() > 0.1
    assert np.abs(J - fd).max() <= 1e-7 * max(1.0, np.abs(J).max()), np.abs(J - fd).max()


def _row_cotangents(con, b, V):
    """Per row of instance b the cotangent on out [V, 3] (sigma folded in)."""
    act = con.active(V)[b]
    w = np.ones(con.C) if con.weight is None else con.weight[b].astype(np.float64)
    for c in range(con.C):
        sigma = np.sqrt(con.fw * w[c]) if act[c] else 0.0
        dirs = [con.normal[b, c].astype(np.float64)] if con.plane else list(np.eye(3))
        for d in dirs:
            g = np.zeros((V, 3))
            if act[c]:
                for i in range(con.S):
                    beta = float(con.barycentric[b, c, i]) if con.S == 3 else 1.0
                    g[con.vertex[b, c, i]] += sigma * beta * d
            yield g


@pytest.mark.parametrize("name,S,plane", CASES)
def test_rows_are_the_composed_backward_passes(name, S, plane):
    rig, skin = RIGS[name]()
    B = 2
    theta, _ = fk.random_inputs(rig, B, 21)
    con = _constraints(len(skin[0]), B, 4, S, plane, 22)
    rt, sk = fk.RigTensors(rig), skr.SkinTensors(*skin, rig.num_joints)
    _, J = vcr.jacobian(rt, sk, theta, con)
    state = fk.skeleton_state(rt, torch.as_tensor(theta.astype(np.float64))).numpy()
    for b in range(B):
        for r, g in enumerate(_row_cotangents(con, b, sk.V)):
            state_grad, _ = skr.vjp_np(skin[0], skin[1], skin[2], skin[3], state[b], g)
            row = fk.vjp_np(rig, theta[b], state[b], state_grad)
            # The channel formulas take the world quaternion as a unit one.  The rigs' pre-rotations are float32 entries, of
            # norm 1 +- 6e-8 each, and the reference composes them as they are: down a chain of depth d the world norm is off
            # by up to d x 6e-8, which is what the two sides may differ by relative to the row (1e-6 covers depth 9 twice
            # over); make_test_character's pre-rotations are exact and agree to rounding.
            tol = 1e-12 if name == "character3" else 1e-6
            assert np.abs(row - J[b, r]).max() <= tol * max(1.0, np.abs(J[b]).max()), (b, r, np.abs(row - J[b, r]).max())


def test_two_sum_form_of_a_column_source():
    """What the kernel evaluates per (constraint, column source): with the influences (joint j, coefficient beta w, posed point
    y) of the constraint and m0 = sum coef, m1 = sum coef y over the influences whose joint lies under the source's joint a,
    d = m1 - m0 t_a: translation m0 tau, rotation omega x d, scale ln 2 d -- equal to the point's column of J."""
    rig, skin = _random_tree()
    joint, weight, inv, rest = skin
    theta, _ = fk.random_inputs(rig, 1, 31)
    con = _constraints(len(joint), 1, 6, 3, False, 32)
    con = vcr.Constraints(con.target, con.vertex, con.barycentric, None, None, 1.0)  # sigma = 1: J is d x_c / d theta
    rt, sk = fk.RigTensors(rig), skr.SkinTensors(*skin, rig.num_joints)
    _, J = vcr.jacobian(rt, sk, theta, con)
    state = fk.skeleton_state(rt, torch.as_tensor(theta.astype(np.float64))).numpy()[0]
    tau, om = fk.axes_np(rig, theta[0], state)
    anc = fk.ancestor_or_self(rig.parent)  # [a, j] = 1: a is j or above it
    invm = skr._inv_np(inv, rig.num_joints)
    for c in range(con.C):
        infl = []
        for i in range(3):
            v = int(con.vertex[0, c, i])
            for k in range(joint.shape[1]):
                if weight[v][k] != 0:
                    j = int(joint[v][k])
                    p = invm[j, :, :3] @ rest[v].astype(np.float64) + invm[j, :, 3]
                    y = state[j, :3] + state[j, 7] * skr.rotation_np(state[j, 3:7]) @ p
                    infl.append((j, float(con.barycentric[0, c, i]) * float(weight[v][k]), y))
        for row in range(7 * rig.num_joints):
            a, d = divmod(row, 7)
            m0 = sum(cf for j, cf, _ in infl if anc[a, j])
            m1 = sum((cf * y for j, cf, y in infl if anc[a, j]), np.zeros(3))
            dd = m1 - m0 * state[a, :3]
            col = m0 * tau[a][:, d] if d < 3 else (np.cross(om[a][:, d - 3], dd) if d < 6 else fk.LN2 * dd)
            for k in range(rig.pt_outer[row], rig.pt_outer[row + 1]):  # (all_dofs_rig: one parameter per row)
                # (1e-6 of the largest entry: the float32 pre-rotations' norms, as in the test above)
                assert np.abs(float(rig.pt_value[k]) * col - J[0, 3 * c : 3 * c + 3, rig.pt_inner[k]]).max() <= 1e-6 * np.abs(J).max()


def test_skipped_constraints_and_enabled_compaction():
    rig, skin = _character3()
    V = len(skin[0])
    B, C = 2, 7
    theta, _ = fk.random_inputs(rig, B, 41)
    con = _constraints(V, B, C, 3, True, 42)
    con.weight[0, 1], con.weight[1, 2], con.weight[0, 3] = 0.0, -1.0, np.nan
    con.vertex[1, 4, 1], con.vertex[0, 5, 2] = -1, V
    con.target[0, 1] = np.nan  # behind a zero weight: not read
    act = con.active(V)
    assert act.sum() == B * C - 5
    full = vcr.normal_equations(rig, skin, theta, con)
    assert np.isfinite(full["H"]).all() and np.isfinite(full["g"]).all() and np.isfinite(full["err"]).all()
    clean = vcr.normal_equations(rig, skin, theta, con.without_skipped(V))
    for key in ("H", "g", "err"):
        assert np.array_equal(full[key], clean[key]), key
    assert (full["r"][~act] == 0).all() and (full["J"][~act] == 0).all()
    enabled = np.ones(rig.num_params, bool)
    enabled[1::3] = False
    sub = vcr.normal_equations(rig, skin, theta, con, enabled=enabled)
    E = np.nonzero(enabled)[0]
    assert np.array_equal(sub["H"], full["H"][:, E][:, :, E]) and np.array_equal(sub["g"], full["g"][:, E])
    assert np.array_equal(sub["err"], full["err"])
    # all weights zero: exact zeros
    zero = vcr.Constraints(con.target, con.vertex, con.barycentric, con.normal, np.zeros((B, C), np.float32), 0.7)
    z = vcr.normal_equations(rig, skin, theta, zero)
    assert not z["H"].any() and not z["g"].any() and not z["err"].any()
