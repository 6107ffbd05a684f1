"""Reference of linear-blend skinning (mmx_skin_points / mmx_skin_points_backward): the forward formula in torch,
parameterised by dtype and differentiable by torch autograd, and a NumPy restatement of the backward pass through the twelve
sums per joint the kernel takes (vjp_np).  Checked on its own in tests/test_skinning_reference.py.

    out[b][v] = sum_k weight[v][k] ( t_j + s_j qrot(q_j, p_vk) ),   p_vk = A_j rest_v + a_j,   j = joint[v][k]

with (t_j, q_j, s_j) the state row [b][j] = (tx,ty,tz, qx,qy,qz,qw, s) and qrot the polynomial of mmx_device.hpp,
p + 2 w (u x p) + 2 u x (u x p): the quaternion is used as the state holds it, never renormalised.  A zero-weight slot is
dropped before any arithmetic (the library's rule: padding contributes nothing, whatever its joint's state holds).
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


def hand_skin(kind):
    """The small hand-made skins of the tests, on make_test_character(3): (joint [V,K], weight [V,K], rest [V,3])."""
    if kind == "character3_k4":  # V = 5, K = 4: zero-weight padding (some of it naming joint 2), joint 2 without influences
        joint = np.array([[0, 1, 2, 2], [1, 0, 2, 0], [0, 2, 2, 2], [1, 1, 2, 0], [0, 1, 0, 1]], np.int32)
        weight = np.array([[0.7, 0.3, 0, 0], [0.25, 0.75, 0, 0], [1.0, 0, 0, 0], [0.5, 0.125, 0, 0.375], [0.4, 0.3, 0.2, 0.1]], np.float32)
        rest = np.array([[0.1, 0.2, -0.3], [0.3, 1.1, 0.2], [-0.2, 0.4, 0.1], [0.05, 1.6, -0.1], [0.2, 0.9, 0.3]], np.float32)
        return joint, weight, rest
    raise KeyError(kind)
