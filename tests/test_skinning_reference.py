"""The skinning reference on its own (CPU): the twelve-sum backward formulas against float64 autograd, the forward against a
plain 4 x 4-matrix linear-blend skinning for unit quaternions, and torch's gradcheck."""
import numpy as np
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


def test_gradcheck():
    joint, weight, inv, rest, state = _random_skin(3, 4, 2, 9)
    sk = ref.SkinTensors(joint, weight, inv, rest, 3)
    st = torch.as_tensor(state[:1]).clone().requires_grad_(True)
    r = torch.as_tensor(rest[None].astype(np.float64)).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda s, x: ref.skin_points(sk, s, x), (st, r), eps=1e-6, atol=1e-7, rtol=1e-6)
