"""Reference of linear-blend skinning (mmx_skin_points / mmx_skin_points_backward): the forward formula in torch,
parameterised by dtype and differentiable by torch autograd, and a NumPy restatement of the backward pass through the twelve
sums per joint the kernel takes (vjp_np).  Checked on its own in tests/test_skinning_reference.py.

    out[b][v] = sum_k weight[v][k] ( t_j + s_j qrot(q_j, p_vk) ),   p_vk = A_j rest_v + a_j,   j = joint[v][k]

with (t_j, q_j, s_j) the state row [b][j] = (tx,ty,tz, qx,qy,qz,qw, s) and qrot the polynomial of mmx_device.hpp,
p + 2 w (u x p) + 2 u x (u x p): the quaternion is used as the state holds it, never renormalised.  A zero-weight slot is
dropped before any arithmetic (the library's rule: padding contributes nothing, whatever its joint's state holds).

Per-entry error bounds (entry_bounds): for every entry of out, rest_grad and state_grad the magnitude its error is measured
against, from the sums of absolute values of the terms that make the entry up, with u = 2^-24 (float32's unit roundoff):
    out[b][v][c]         |x - x64| <= (K + 7) u A,   A = sum_k |w| ( sum_d |sRA_j[c][d]| |rest_d| + |(sRa_j)_c| + |t_j,c| )
        one rounding of the posed affine M_j (built in double), at most four in a row's dot product, one product with the
        weight and at most K accumulations: gamma_(K+6) < (K + 7) u.
    rest_grad[b][v][c]   the same with the 3 x 3 part transposed, the cotangent in the place of rest and no translation term.
    state_grad[b][j][c]  |x - x64| <= u |x64| + (n_j + 64) 2^-52 S,   n_j the joint's entry count and S the twelve-sum formulas
        of vjp_np with every factor replaced by its absolute value and every subtraction by an addition: the sums are taken in
        double from the float32 entries the reference reads and each channel is rounded once.  S = 0 asks for a zero (of
        either sign): a joint without entries, the q channels at scale 0 or at the zero quaternion.
tests/test_skinning_reference.py shows on the CPU that restatements of the kernels' arithmetic hold the rules and that a float32
accumulation or a transposed N breaks the state rule.
"""
import numpy as np
import torch


def qrot(q, v):
    u, w = q[..., :3], q[..., 3:]
    uv = 2.0 * torch.cross(u, v, dim=-1)
    return v + w * uv + torch.cross(u, uv, dim=-1)


class SkinTensors:
    """A skin's arrays as torch tensors of one dtype / device (float32 entries, exactly)."""

    def __init__(self, joint, weight, inverse_bind, rest, num_joints, dtype=torch.float64, device="cpu"):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype, device=device)
        self.dtype, self.device = dtype, device
        self.joint = torch.as_tensor(np.asarray(joint, np.int64), device=device)  # [V, K]
        self.weight = t(weight)  # [V, K]
        ib = np.tile(np.eye(3, 4).reshape(1, 12), (num_joints, 1)) if inverse_bind is None else np.asarray(inverse_bind)
        self.inv = t(ib).reshape(num_joints, 3, 4)
        self.rest = t(rest)  # [V, 3]
        self.J, (self.V, self.K) = int(num_joints), self.joint.shape


def skin_points(sk: SkinTensors, state, rest=None):
    """state [B, J, 8], rest None (the skin's) or [B, V, 3] -> vertices [B, V, 3].  The gather-and-blend a caller writes in
    torch: one gather of the joint rows per slot, [B, V, K, 3] temporaries."""
    B = state.shape[0]
    r = sk.rest.unsqueeze(0).expand(B, -1, -1) if rest is None else rest  # [B, V, 3]
    A, a = sk.inv[sk.joint][..., :3], sk.inv[sk.joint][..., 3]  # [V, K, 3, 3], [V, K, 3]
    p = torch.einsum("vkij,bvj->bvki", A, r) + a.unsqueeze(0)  # [B, V, K, 3]
    rows = state[:, sk.joint]  # [B, V, K, 8]
    posed = rows[..., :3] + rows[..., 7:8] * qrot(rows[..., 3:7], p)
    w = sk.weight.unsqueeze(0).unsqueeze(-1)  # [1, V, K, 1]
    return torch.where(w != 0, w * posed, torch.zeros((), dtype=posed.dtype, device=posed.device)).sum(2)


def vjp_autograd(sk: SkinTensors, state, cot, rest=None):
    """(out, d sum(cot * out) / d state [B, J, 8], d / d rest [B, V, 3]) by torch autograd, as numpy.  The rest gradient is
    with respect to per-instance rest positions (the skin's own repeated B times when rest is None)."""
    st = torch.as_tensor(np.asarray(state), dtype=sk.dtype, device=sk.device).clone().requires_grad_(True)
    B = st.shape[0]
    r0 = sk.rest.unsqueeze(0).expand(B, -1, -1) if rest is None else torch.as_tensor(np.asarray(rest), dtype=sk.dtype, device=sk.device)
    r = r0.clone().requires_grad_(True)
    out = skin_points(sk, st, r)
    (out * torch.as_tensor(np.asarray(cot), dtype=sk.dtype, device=sk.device)).sum().backward()
    return out.detach().cpu().numpy(), st.grad.cpu().numpy(), r.grad.cpu().numpy()


def rotation_np(q):
    """R(q) of the polynomial for any q = (u, w): (1 - 2 |u|^2) I + 2 u u^T + 2 w [u]x."""
    u, w = q[:3], q[3]
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return (1.0 - 2.0 * (u @ u)) * np.eye(3) + 2.0 * np.outer(u, u) + 2.0 * w * K


def vjp_np(joint, weight, inverse_bind, rest, state, g):
    """One instance: state [J, 8], rest [V, 3], g = dL/dout [V, 3] -> (state_grad [J, 8], rest_grad [V, 3]) in float64, from
    the twelve sums per joint F = sum w g, N = sum w g p^T:  g_t = F,  g_s = <R(q), N>,  g_q = s d<R(q), N>/dq with
    <R(q), N> = (1 - 2 |u|^2) tr N + 2 u^T N u + 2 w u . ax(N),  ax(N) = (N21 - N12, N02 - N20, N10 - N01)."""
    state, rest, g = (np.asarray(x, np.float64) for x in (state, rest, g))
    J = state.shape[0]
    inv = (np.tile(np.eye(3, 4).reshape(1, 12), (J, 1)) if inverse_bind is None else np.asarray(inverse_bind, np.float64)).reshape(J, 3, 4)
    V, K = np.asarray(joint).shape
    F, N = np.zeros((J, 3)), np.zeros((J, 3, 3))
    used = np.zeros(J, bool)
    rest_grad = np.zeros((V, 3))
    for v in range(V):
        for k in range(K):
            w, j = float(weight[v][k]), int(joint[v][k])
            if w == 0.0:
                continue
            used[j] = True
            p = inv[j, :, :3] @ rest[v] + inv[j, :, 3]
            F[j] += w * g[v]
            N[j] += w * np.outer(g[v], p)
            rest_grad[v] += w * inv[j, :, :3].T @ (state[j, 7] * rotation_np(state[j, 3:7]).T @ g[v])
    out = np.zeros((J, 8))
    for j in np.nonzero(used)[0]:
        u, qw, s = state[j, 3:6], state[j, 6], state[j, 7]
        n = N[j]
        tr, ax = np.trace(n), np.array([n[2, 1] - n[1, 2], n[0, 2] - n[2, 0], n[1, 0] - n[0, 1]])
        out[j, :3] = F[j]
        out[j, 3:6] = s * (-4.0 * tr * u + 2.0 * (n + n.T) @ u + 2.0 * qw * ax)
        out[j, 6] = s * 2.0 * (u @ ax)
        out[j, 7] = (1.0 - 2.0 * (u @ u)) * tr + 2.0 * u @ n @ u + 2.0 * qw * (u @ ax)
    return out, rest_grad


def lbs_matrices_np(joint, weight, inverse_bind, rest, state):
    """Plain 4 x 4-matrix linear-blend skinning for UNIT quaternions (one instance, float64): sum_k w T_world,j T_invbind,j r."""
    state, rest = np.asarray(state, np.float64), np.asarray(rest, np.float64)
    J = state.shape[0]
    inv = (np.tile(np.eye(3, 4).reshape(1, 12), (J, 1)) if inverse_bind is None else np.asarray(inverse_bind, np.float64)).reshape(J, 3, 4)
    mats = []
    for j in range(J):
        x, y, z, w = state[j, 3:7]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])  # fmt: skip
        Tw, Ti = np.eye(4), np.eye(4)
        Tw[:3, :3], Tw[:3, 3] = state[j, 7] * R, state[j, :3]
        Ti[:3] = inv[j]
        mats.append(Tw @ Ti)
    out = np.zeros((rest.shape[0], 3))
    for v in range(rest.shape[0]):
        for k in range(np.asarray(joint).shape[1]):
            out[v] += float(weight[v][k]) * (mats[int(joint[v][k])] @ np.append(rest[v], 1.0))[:3]
    return out


U32 = 2.0**-24  # float32's unit roundoff


def _inv_np(inverse_bind, J):
    return (np.tile(np.eye(3, 4).reshape(1, 12), (J, 1)) if inverse_bind is None else np.asarray(inverse_bind, np.float64)).reshape(J, 3, 4)


def _entries(joint, weight):
    """(vertex, joint, weight) of every non-zero-weight slot, in (vertex, slot) order."""
    joint, weight = np.asarray(joint), np.asarray(weight, np.float64)
    v, k = np.nonzero(weight != 0)
    return v, joint[v, k].astype(np.int64), weight[v, k]


def _rest_b(rest, B):
    rest = np.asarray(rest, np.float64)
    return np.broadcast_to(rest, (B,) + rest.shape[-2:]) if rest.ndim == 2 else rest


def arbitrary_states(J, B, seed, used=None):
    """[B, J, 8] float32 states no forward kinematics gives: translations N(0, 10); unit quaternions times a norm factor in
    [0.5, 2] times a random sign; scales drawn from {-1.5, 2^-20, 1, 3}.  Four rows are planted on (instance, joint) pairs with
    the joint in `used` (the joints that have entries; default: all): the zero quaternion, (0, 0, 0, w), scale exactly 0 and
    scale -1.5 -- on distinct pairs where there are four."""
    rng = np.random.default_rng(seed)
    st = np.zeros((B, J, 8))
    st[..., :3] = rng.normal(0.0, 10.0, size=(B, J, 3))
    q = rng.normal(size=(B, J, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    st[..., 3:7] = q * rng.uniform(0.5, 2.0, size=(B, J, 1)) * rng.choice([-1.0, 1.0], size=(B, J, 1))
    st[..., 7] = rng.choice([-1.5, 2.0**-20, 1.0, 3.0], size=(B, J))
    used = np.arange(J) if used is None else np.asarray(used)
    pairs = [(b, int(j)) for j in used for b in range(B)]
    assert len(pairs) >= 2
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    at = lambda i: pairs[i % len(pairs)]
    st[at(0)][3:7] = 0.0
    st[at(1)][3:6] = 0.0
    st[at(2)][7] = 0.0
    st[at(3)][7] = -1.5
    return st.astype(np.float32)


def posed_affines_np(inverse_bind, state):
    """state [B, J, 8] -> (s R(q) A_j [B, J, 3, 3], s R(q) a_j [B, J, 3]) in float64; the posed affine is [sRA | sRa + t]."""
    state = np.asarray(state, np.float64)
    inv = _inv_np(inverse_bind, state.shape[1])
    u, w, s = state[..., 3:6], state[..., 6], state[..., 7]
    K = np.zeros(state.shape[:2] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -u[..., 2], u[..., 1], u[..., 2], -u[..., 0], -u[..., 1], u[..., 0]
    R = (1.0 - 2.0 * (u * u).sum(-1))[..., None, None] * np.eye(3) + 2.0 * u[..., :, None] * u[..., None, :] + 2.0 * w[..., None, None] * K
    sR = s[..., None, None] * R
    return sR @ inv[:, :, :3], np.einsum("bjcd,jd->bjc", sR, inv[:, :, 3])


def twelve_sums_np(joint, weight, inverse_bind, rest, g, J, acc=np.float64):
    """F [B, J, 3] = sum w g and N [B, J, 3, 3] = sum w g p^T over every joint's entries, for rest [V, 3] or [B, V, 3] and
    g [B, V, 3]: the terms in float64, accumulated entry after entry in `acc`."""
    g = np.asarray(g, np.float64)
    B = g.shape[0]
    inv = _inv_np(inverse_bind, J)
    v, je, we = _entries(joint, weight)
    p = np.einsum("ecd,bed->bec", inv[je, :, :3], _rest_b(rest, B)[:, v]) + inv[je, :, 3]
    wg = we[None, :, None] * g[:, v]
    F, N = np.zeros((B, J, 3), acc), np.zeros((B, J, 3, 3), acc)
    np.add.at(F, (slice(None), je), wg.astype(acc))
    np.add.at(N, (slice(None), je), (wg[..., :, None] * p[..., None, :]).astype(acc))
    return F.astype(np.float64), N.astype(np.float64)


def state_channels_np(F, N, state):
    """The eight channels [B, J, 8] from the twelve sums (the formulas of vjp_np), in float64."""
    state = np.asarray(state, np.float64)
    u, qw, s = state[..., 3:6], state[..., 6], state[..., 7]
    tr = np.trace(N, axis1=-2, axis2=-1)
    ax = np.stack([N[..., 2, 1] - N[..., 1, 2], N[..., 0, 2] - N[..., 2, 0], N[..., 1, 0] - N[..., 0, 1]], -1)
    nu, ntu = np.einsum("bjcd,bjd->bjc", N, u), np.einsum("bjdc,bjd->bjc", N, u)
    uax = (u * ax).sum(-1)
    out = np.zeros(state.shape)
    out[..., :3] = F
    out[..., 3:6] = s[..., None] * (-4.0 * tr[..., None] * u + 2.0 * (nu + ntu) + 2.0 * qw[..., None] * ax)
    out[..., 6] = s * 2.0 * uax
    out[..., 7] = (1.0 - 2.0 * (u * u).sum(-1)) * tr + 2.0 * (u * nu).sum(-1) + 2.0 * qw * uax
    return out


def state_grad_np(joint, weight, inverse_bind, rest, state, g, acc=np.float64):
    """vjp_np's state gradient for a batch, vectorised: [B, J, 8] float64; a joint without entries gets zeros whatever its row."""
    J = np.asarray(state).shape[1]
    F, N = twelve_sums_np(joint, weight, inverse_bind, rest, g, J, acc)
    used = np.bincount(_entries(joint, weight)[1], minlength=J) > 0
    st = np.where(used[None, :, None], np.asarray(state, np.float64), 0.0)
    return np.where(used[None, :, None], state_channels_np(F, N, st), 0.0)


def entry_bounds(joint, weight, inverse_bind, rest, state, g):
    """The magnitudes of the per-entry rules (module docstring) for state [B, J, 8], rest [V, 3] or [B, V, 3] and the cotangent
    g [B, V, 3]: dict(out=A [B, V, 3], rest_grad=A [B, V, 3], state_grad=S [B, J, 8], entries=n_j [J]).  Zero-weight slots are
    omitted everywhere; a joint without entries may hold anything."""
    state, g = np.asarray(state, np.float64), np.abs(np.asarray(g, np.float64))
    joint, weight = np.asarray(joint), np.abs(np.asarray(weight, np.float64))
    B, J = state.shape[:2]
    inv = np.abs(_inv_np(inverse_bind, J))
    r = np.abs(_rest_b(rest, B))
    v, je, we = _entries(joint, weight)
    n = np.bincount(je, minlength=J)
    st = np.where((n > 0)[None, :, None], state, 0.0)
    sRA, sRa = (np.abs(x) for x in posed_affines_np(inverse_bind, st))
    t = np.abs(st[..., :3])
    A_out, A_rest = np.zeros((B, len(joint), 3)), np.zeros((B, len(joint), 3))
    np.add.at(A_out, (slice(None), v), we[None, :, None] * (np.einsum("becd,bed->bec", sRA[:, je], r[:, v]) + sRa[:, je] + t[:, je]))
    np.add.at(A_rest, (slice(None), v), we[None, :, None] * np.einsum("bedc,bed->bec", sRA[:, je], g[:, v]))
    # the twelve sums of absolute values and the channels with every sign turned to plus
    p = np.einsum("ecd,bed->bec", inv[je, :, :3], r[:, v]) + inv[je, :, 3]
    wg = we[None, :, None] * g[:, v]
    F, N = np.zeros((B, J, 3)), np.zeros((B, J, 3, 3))
    np.add.at(F, (slice(None), je), wg)
    np.add.at(N, (slice(None), je), wg[..., :, None] * p[..., None, :])
    u, qw, s = np.abs(st[..., 3:6]), np.abs(st[..., 6]), np.abs(st[..., 7])
    tr = np.trace(N, axis1=-2, axis2=-1)
    ax = np.stack([N[..., 2, 1] + N[..., 1, 2], N[..., 0, 2] + N[..., 2, 0], N[..., 1, 0] + N[..., 0, 1]], -1)
    nu, ntu = np.einsum("bjcd,bjd->bjc", N, u), np.einsum("bjdc,bjd->bjc", N, u)
    uax = (u * ax).sum(-1)
    S = np.zeros((B, J, 8))
    S[..., :3] = F
    S[..., 3:6] = s[..., None] * (4.0 * tr[..., None] * u + 2.0 * (nu + ntu) + 2.0 * qw[..., None] * ax)
    S[..., 6] = 2.0 * s * uax
    S[..., 7] = (1.0 + 2.0 * (u * u).sum(-1)) * tr + 2.0 * (u * nu).sum(-1) + 2.0 * qw * uax
    return dict(out=A_out, rest_grad=A_rest, state_grad=S, entries=n)


def entry_ratios(key, got, want64, bounds, K):
    """Per entry, the error over what its rule allows (<= 1 holds the rule; an entry whose magnitude is 0 must be a zero and
    gets 0 or inf): out / rest_grad err / ((K + 7) u A), state_grad (err - u |x64|) / ((n_j + 64) 2^-52 S)."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    err = np.abs(got - want64)
    if key == "state_grad":
        num, den = err - U32 * np.abs(want64), (bounds["entries"][None, :, None] + 64.0) * 2.0**-52 * bounds["state_grad"]
    else:
        num, den = err, (K + 7) * U32 * bounds[key]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where((got == 0) & (want64 == 0), 0.0, np.inf))


def hand_skin(kind):
    """The small hand-made skins of the tests, on make_test_character(3): (joint [V,K], weight [V,K], rest [V,3])."""
    if kind == "character3_k4":  # V = 5, K = 4: zero-weight padding (some of it naming joint 2), joint 2 without influences
        joint = np.array([[0, 1, 2, 2], [1, 0, 2, 0], [0, 2, 2, 2], [1, 1, 2, 0], [0, 1, 0, 1]], np.int32)
        weight = np.array([[0.7, 0.3, 0, 0], [0.25, 0.75, 0, 0], [1.0, 0, 0, 0], [0.5, 0.125, 0, 0.375], [0.4, 0.3, 0.2, 0.1]], np.float32)
        rest = np.array([[0.1, 0.2, -0.3], [0.3, 1.1, 0.2], [-0.2, 0.4, 0.1], [0.05, 1.6, -0.1], [0.2, 0.9, 0.3]], np.float32)
        return joint, weight, rest
    raise KeyError(kind)
