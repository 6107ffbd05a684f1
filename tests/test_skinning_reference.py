"""The skinning reference on its own (CPU): the twelve-sum backward formulas against float64 autograd, the forward against a
plain 4 x 4-matrix linear-blend skinning for unit quaternions, and torch's gradcheck.  And the per-entry error rules of
ref.entry_bounds: restatements of the kernels' arithmetic (double sums rounded once; the float32 blend in the kernel's order) hold
them, a float32 accumulation of the sums and N u in the place of N^T u break them -- on forward-kinematics and arbitrary states."""
import numpy as np
import pytest
import torch

from tests import skinning_reference as ref


def _random_skin(J, V, K, seed, unit=False):
    rng = np.random.default_rng(seed)
    joint = rng.integers(0, J, size=(V, K)).astype(np.int32)
    weight = rng.uniform(0.1, 1.0, size=(V, K)).astype(np.float32)
    weight[rng.uniform(size=(V, K)) < 0.25] = 0.0  # padding
    weight[:, 0] = np.maximum(weight[:, 0], 0.1)
    inv = rng.normal(size=(J, 12)).astype(np.float32)
    rest = rng.normal(size=(V, 3)).astype(np.float32)
    state = rng.normal(size=(2, J, 8))
    state[..., 7] = rng.uniform(0.7, 1.4, size=(2, J))
    if unit:
        state[..., 3:7] /= np.linalg.norm(state[..., 3:7], axis=-1, keepdims=True)
    return joint, weight, inv, rest, state


def test_twelve_sum_formulas_match_autograd():
    """Non-unit quaternions on purpose: the derivative is that of the polynomial, with no renormalisation term."""
    for J, V, K, seed in ((3, 5, 4, 1), (7, 40, 8, 2), (1, 1, 1, 3)):
        joint, weight, inv, rest, state = _random_skin(J, V, K, seed)
        cot = np.random.default_rng(seed + 10).normal(size=(2, V, 3))
        sk = ref.SkinTensors(joint, weight, inv, rest, J)
        _, sg, rg = ref.vjp_autograd(sk, state, cot)
        for b in range(2):
            got_s, got_r = ref.vjp_np(joint, weight, inv, rest, state[b], cot[b])
            assert np.abs(got_s - sg[b]).max() <= 1e-12 * np.abs(sg[b]).max()
            assert np.abs(got_r - rg[b]).max() <= 1e-12 * np.abs(rg[b]).max()
        # per-instance rest positions: the same formulas on that instance's rest
        rest_b = rest[None] + 0.1 * np.random.default_rng(seed + 20).normal(size=(2, V, 3))
        _, sg, rg = ref.vjp_autograd(sk, state, cot, rest_b)
        for b in range(2):
            got_s, got_r = ref.vjp_np(joint, weight, inv, rest_b[b], state[b], cot[b])
            assert np.abs(got_s - sg[b]).max() <= 1e-12 * np.abs(sg[b]).max()
            assert np.abs(got_r - rg[b]).max() <= 1e-12 * np.abs(rg[b]).max()


def test_forward_is_matrix_lbs_for_unit_quaternions():
    joint, weight, inv, rest, state = _random_skin(6, 30, 4, 5, unit=True)
    sk = ref.SkinTensors(joint, weight, inv, rest, 6)
    out = ref.skin_points(sk, torch.as_tensor(state)).numpy()
    for b in range(2):
        want = ref.lbs_matrices_np(joint, weight, inv, rest, state[b])
        assert np.abs(out[b] - want).max() <= 1e-12 * np.abs(want).max()
    # no inverse bind = identity
    sk0 = ref.SkinTensors(joint, weight, None, rest, 6)
    want = ref.lbs_matrices_np(joint, weight, None, rest, state[0])
    assert np.abs(ref.skin_points(sk0, torch.as_tensor(state))[0].numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_zero_weight_slot_contributes_nothing():
    joint, weight, rest = ref.hand_skin("character3_k4")
    assert not ((joint == 2) & (weight != 0)).any() and (joint == 2).any()
    state = np.random.default_rng(7).normal(size=(1, 3, 8))
    sk = ref.SkinTensors(joint, weight, None, rest, 3)
    base = ref.skin_points(sk, torch.as_tensor(state)).numpy()
    state[0, 2] = np.nan
    assert np.array_equal(ref.skin_points(sk, torch.as_tensor(state)).numpy(), base)
    sg, _ = ref.vjp_np(joint, weight, None, rest, state[0], np.ones((5, 3)))
    assert np.all(sg[2] == 0.0) and np.isfinite(sg).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the per-entry rules of ref.entry_bounds: sound for restatements of the kernels' arithmetic, broken by subtly wrong ones
# ---------------------------------------------------------------------------------------------------------------------------
def _bound_case(rig_name, states):
    """(skin, state [3, J, 8] float32, cotangent, float64 autograd reference, bounds) -- built once per case."""
    key = (rig_name, states)
    if key not in _bound_cases:
        from momentum_amd import make_humanoid72, make_test_character, make_test_skin
        from tests import skeleton_state_reference as fk

        if rig_name == "humanoid72":
            rig = make_humanoid72(variant="p128", unit=0.01)
            skin = make_test_skin(rig, 600, 4, 42)
        else:
            rig = make_test_character(24)
            skin = make_test_skin(rig, 300, 8, 41, random_affine=True)
        B, J = 3, rig.num_joints
        if states == "fk":
            theta, _ = fk.random_inputs(rig, B, seed=11)
            state = fk.skeleton_state(fk.RigTensors(rig), torch.as_tensor(theta, dtype=torch.float64)).numpy().astype(np.float32)
        else:
            state = ref.arbitrary_states(J, B, seed=12, used=np.unique(skin.joint[skin.weight != 0]))
        cot = np.random.default_rng(13).normal(size=(B, skin.joint.shape[0], 3)).astype(np.float32)
        sk = ref.SkinTensors(skin.joint, skin.weight, skin.inverse_bind, skin.rest, J)
        want = dict(zip(("out", "state_grad", "rest_grad"), ref.vjp_autograd(sk, state, cot)))
        _bound_cases[key] = (skin, state, cot, want, ref.entry_bounds(skin.joint, skin.weight, skin.inverse_bind, skin.rest, state, cot))
    return _bound_cases[key]


_bound_cases = {}
BOUND_CASES = [(r, s) for r in ("humanoid72", "character24_k8") for s in ("fk", "arbitrary")]


def _forward_f32(skin, state, x, transposed):
    """The forward kernel's arithmetic in float32: the posed affine built in float64 and rounded once, a row's dot product left
    to right, the product with the weight, the slots accumulated in order; transposed: the rest gradient's form."""
    f = np.float32
    sRA, sRa = ref.posed_affines_np(skin.inverse_bind, state)
    M, m3 = sRA.astype(f), (sRa + state[..., :3].astype(np.float64)).astype(f)
    x = np.broadcast_to(np.asarray(x, f), (state.shape[0],) + x.shape[-2:])
    acc = np.zeros(x.shape, f)
    for k in range(skin.joint.shape[1]):
        Mk, w = M[:, skin.joint[:, k]], skin.weight[None, :, k, None].astype(f)  # [B, V, 3, 3]
        if transposed:
            p = Mk[..., 0, :] * x[..., 0:1] + Mk[..., 1, :] * x[..., 1:2] + Mk[..., 2, :] * x[..., 2:3]
        else:
            p = Mk[..., :, 0] * x[..., 0:1] + Mk[..., :, 1] * x[..., 1:2] + Mk[..., :, 2] * x[..., 2:3] + m3[:, skin.joint[:, k]]
        assert p.dtype == f
        acc = acc + np.where(w != 0, w * p, f(0))
    return acc


def test_arbitrary_states_are_what_they_say():
    used = np.array([1, 4, 5])
    st = ref.arbitrary_states(7, 3, 5, used=used)
    assert st.dtype == np.float32 and st.shape == (3, 7, 8) and np.isfinite(st).all()
    assert np.array_equal(st, ref.arbitrary_states(7, 3, 5, used=used))
    norm = np.linalg.norm(st[..., 3:7].astype(np.float64), axis=-1)
    on = st[:, used]
    full = np.abs(st[..., 3:6]).max(-1) > 0  # (the two planted rows aside)
    assert (norm == 0).sum() == 1 and (~full).sum() == 2 and ((norm[full] < 0.499) | (norm[full] > 2.001)).sum() == 0
    assert (np.linalg.norm(on[..., 3:7], axis=-1) == 0).sum() == 1  # the zero quaternion, on a joint that has entries
    assert ((np.abs(on[..., 3:6]).max(-1) == 0) & (on[..., 6] != 0)).sum() == 1  # (0, 0, 0, w)
    assert (on[..., 7] == 0).sum() == 1 and (on[..., 7] == -1.5).sum() >= 1
    assert set(np.unique(st[..., 7])) <= {-1.5, 0.0, 2.0**-20, 1.0, 3.0}
    assert (st[..., 3:7] < 0).any() and np.abs(st[..., :3]).max() > 10.0


@pytest.mark.parametrize("rig_name,states", BOUND_CASES)
def test_double_sums_rounded_once_hold_the_state_rule(rig_name, states):
    skin, state, cot, want, bounds = _bound_case(rig_name, states)
    got = ref.state_grad_np(skin.joint, skin.weight, skin.inverse_bind, skin.rest, state, cot).astype(np.float32)
    err = np.abs(got.astype(np.float64) - want["state_grad"])
    print(f"{rig_name}/{states}: max(err - u|ref|) {np.max(err - ref.U32 * np.abs(want['state_grad'])):.3e}")
    assert np.max(err - ref.U32 * np.abs(want["state_grad"])) <= 0.0
    assert ref.entry_ratios("state_grad", got, want["state_grad"], bounds, skin.joint.shape[1]).max() <= 1.0
    # the vectorised sums are vjp_np's
    one, _ = ref.vjp_np(skin.joint, skin.weight, skin.inverse_bind, skin.rest, state[1], cot[1])
    full = ref.state_grad_np(skin.joint, skin.weight, skin.inverse_bind, skin.rest, state, cot)[1]
    assert np.abs(full - one).max() <= 1e-13 * np.abs(one).max()
    # S = 0: the reference holds an exact zero there, and only there is S zero on a joint that has entries
    S, n = bounds["state_grad"], bounds["entries"]
    assert np.all(want["state_grad"][S == 0] == 0.0)
    if states == "arbitrary":
        assert (S[:, n > 0] == 0).any() and (S[:, n > 0, :3] > 0).all()


@pytest.mark.parametrize("rig_name,states", BOUND_CASES)
def test_float32_forward_in_kernel_order_holds_the_forward_rules(rig_name, states):
    skin, state, cot, want, bounds = _bound_case(rig_name, states)
    K = skin.joint.shape[1]
    for key, got in (("out", _forward_f32(skin, state, skin.rest, False)), ("rest_grad", _forward_f32(skin, state, cot, True))):
        r = ref.entry_ratios(key, got, want[key], bounds, K)
        print(f"{rig_name}/{states}/{key}: worst err / (u A) {r.max() * (K + 7):.2f} of {K + 7}")
        assert r.max() <= 1.0, key


@pytest.mark.parametrize("rig_name,states", BOUND_CASES)
def test_float32_accumulation_breaks_the_state_rule(rig_name, states):
    """The teeth: F and N accumulated in float32 (channels in double, rounded once) -- inside the per-instance max-norm
    yardstick of tests/test_gpu_skin_points.py, outside the per-entry rule."""
    skin, state, cot, want, bounds = _bound_case(rig_name, states)
    got = ref.state_grad_np(skin.joint, skin.weight, skin.inverse_bind, skin.rest, state, cot, acc=np.float32).astype(np.float32)
    r = ref.entry_ratios("state_grad", got, want["state_grad"], bounds, skin.joint.shape[1])
    share = (r > 1.0).mean()
    print(f"{rig_name}/{states}: {int((r > 1.0).sum())} of {r.size} entries over the rule, worst {r.max():.0f} x")
    assert r.max() > 1.0
    if rig_name == "humanoid72":
        assert share >= 0.1, share


@pytest.mark.parametrize("rig_name,states", BOUND_CASES)
def test_n_for_its_transpose_breaks_the_state_rule(rig_name, states):
    """The teeth: N u in the place of N^T u in dphi/du, everything in double."""
    skin, state, cot, want, bounds = _bound_case(rig_name, states)
    J = state.shape[1]
    F, N = ref.twelve_sums_np(skin.joint, skin.weight, skin.inverse_bind, skin.rest, cot, J)
    st = state.astype(np.float64)
    u, qw, s = st[..., 3:6], st[..., 6], st[..., 7]
    ax = np.stack([N[..., 2, 1] - N[..., 1, 2], N[..., 0, 2] - N[..., 2, 0], N[..., 1, 0] - N[..., 0, 1]], -1)
    nu = np.einsum("bjcd,bjd->bjc", N, u)
    got = ref.state_channels_np(F, N, st)
    assert np.abs(got - want["state_grad"]).max() <= 1e-12 * np.abs(want["state_grad"]).max()
    got[..., 3:6] = s[..., None] * (-4.0 * np.trace(N, axis1=-2, axis2=-1)[..., None] * u + 2.0 * (nu + nu) + 2.0 * qw[..., None] * ax)
    r = ref.entry_ratios("state_grad", got.astype(np.float32), want["state_grad"], bounds, skin.joint.shape[1])
    print(f"{rig_name}/{states}: worst {r.max():.3g} x, channels over the rule {sorted(set(np.nonzero(r > 1.0)[2].tolist()))}")
    assert r.max() > 1.0 and set(np.nonzero(r > 1.0)[2].tolist()) <= {3, 4, 5}


def test_gradcheck():
    joint, weight, inv, rest, state = _random_skin(3, 4, 2, 9)
    sk = ref.SkinTensors(joint, weight, inv, rest, 3)
    st = torch.as_tensor(state[:1]).clone().requires_grad_(True)
    r = torch.as_tensor(rest[None].astype(np.float64)).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda s, x: ref.skin_points(sk, s, x), (st, r), eps=1e-6, atol=1e-7, rtol=1e-6)
