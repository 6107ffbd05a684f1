"""Live-joint bookkeeping of mmx_tuning::joint_pruning on the CPU (mmx_host_live_joints): the joints a problem's solve
can depend on are the ancestors-or-self of the joints it references; they are renumbered by maps that are monotone in
joint index and in DFS position, so that every sum over joints keeps its order."""
import numpy as np
import pytest

from momentum_amd import capi, humanoid72_landmark_joints, make_humanoid72
from momentum_amd.rigs import _build_rig


def tree(parent):
    """A rig with the given parents and one rotation parameter per joint (the bookkeeping reads the parents only)."""
    J = len(parent)
    pre = np.zeros((J, 4), np.float32)
    pre[:, 3] = 1.0
    off = np.full((J, 3), 0.1, np.float32)
    trip = [(7 * j + 3, j, 1.0) for j in range(J)]
    return _build_rig(parent, pre, off, trip, J, [f"j{j}" for j in range(J)], [f"p{j}" for j in range(J)])


def live_reference(parent, joints):
    """The rule restated: mark every referenced joint and its ancestors; nothing referenced = nothing pruned."""
    J = len(parent)
    live = np.zeros(J, np.uint8)
    for j in joints:
        while j >= 0 and not live[j]:
            live[j] = 1
            j = int(parent[j])
    if not live.any():
        live[:] = 1
    compact = np.where(live == 1, np.cumsum(live) - 1, -1).astype(np.int32)
    return live, compact, int(live.sum())


def check(rig, joints):
    out = capi.host_live_joints(rig, joints)
    live, compact, n = live_reference(rig.parent, joints)
    assert out["num_live"] == n
    assert np.array_equal(out["live"], live)
    assert np.array_equal(out["compact_of"], compact)
    kept = np.flatnonzero(live)
    # monotone in joint index ...
    assert np.all(np.diff(compact[kept]) == 1) and compact[kept[0]] == 0
    # ... and in DFS position: the rig over the live joints (a live joint's parent is live) visits them in the order the full
    # rig does, and a live joint's subtree is the live part of its full subtree
    assert all(rig.parent[j] < 0 or live[rig.parent[j]] for j in kept)
    sub = tree([-1 if rig.parent[j] < 0 else int(compact[rig.parent[j]]) for j in kept])
    full_t, sub_t = capi.host_tables(rig), capi.host_tables(sub)
    by_full_pos = kept[np.argsort(full_t["tin"][kept])]
    assert np.array_equal(sub_t["tin"][compact[by_full_pos]], np.arange(n))
    for j in kept:
        inside = [k for k in kept if full_t["tin"][j] <= full_t["tin"][k] < full_t["tout"][j]]
        assert sub_t["tout"][compact[j]] - sub_t["tin"][compact[j]] == len(inside)
    return out


def test_chain_with_the_constraint_mid_chain():
    rig = tree([-1, 0, 1, 2, 3, 4, 5])
    out = check(rig, [3])
    assert out["num_live"] == 4 and list(out["compact_of"]) == [0, 1, 2, 3, -1, -1, -1]


def test_star():
    rig = tree([-1, 0, 0, 0, 0, 0])
    out = check(rig, [4, 2])
    assert list(out["live"]) == [1, 0, 1, 0, 1, 0] and list(out["compact_of"]) == [0, -1, 1, -1, 2, -1]


def test_humanoid72_with_its_landmarks_keeps_41_joints():
    rig = make_humanoid72(variant="p128")
    lm = humanoid72_landmark_joints(rig)
    assert len(lm) == 16
    out = check(rig, lm)
    assert out["num_live"] == 41
    dead = [n for n, l in zip(rig.joint_names, out["live"]) if not l]
    assert len(dead) == 31
    for name in dead:
        assert name == "jaw" or name.startswith(("eye_", "toe_end_", "forearm_twist_", "middle", "ring", "pinky")), name
    for name, l in zip(rig.joint_names, out["live"]):
        if name == "jaw" or name.startswith(("eye_", "toe_end_", "forearm_twist_", "middle", "ring", "pinky")):
            assert not l, name


def test_dead_subtree_between_two_live_siblings():
    #        0
    #   1    3    6        (3's subtree 3, 4, 5 is dead; 6's positions shift by three)
    #   2   4 5   7
    rig = tree([-1, 0, 1, 0, 3, 3, 0, 6])
    out = check(rig, [2, 7])
    assert list(out["compact_of"]) == [0, 1, 2, -1, -1, -1, 3, 4]
    t = capi.host_tables(rig)
    assert t["tin"][6] == 6  # behind the dead subtree in the full rig, position 3 among the live ones (checked in check())


def test_two_roots_with_one_tree_entirely_dead():
    rig = tree([-1, 0, 1, -1, 3, 4])
    out = check(rig, [5])
    assert list(out["live"]) == [0, 0, 0, 1, 1, 1] and list(out["compact_of"]) == [-1, -1, -1, 0, 1, 2]
    out = check(rig, [1])
    assert list(out["compact_of"]) == [0, 1, -1, -1, -1, -1]


def test_all_joints_referenced_is_the_identity():
    rig = tree([-1, 0, 0, 1, 1, 2])
    out = check(rig, [3, 4, 5])
    assert out["num_live"] == 6 and list(out["compact_of"]) == list(range(6))


def test_no_joint_referenced_is_the_identity():
    rig = tree([-1, 0, 0, 1, 1, 2])
    out = check(rig, [])
    assert out["num_live"] == 6 and list(out["live"]) == [1] * 6 and list(out["compact_of"]) == list(range(6))


def test_out_of_range_joint_is_refused():
    rig = tree([-1, 0, 1])
    with pytest.raises(capi.MmxError):
        capi.host_live_joints(rig, [3])
