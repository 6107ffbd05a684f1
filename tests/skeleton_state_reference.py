"""Reference of the skeleton state and of its derivative (test infrastructure).

skeleton_state(rig, theta): a pure-torch forward kinematics, differentiable by torch autograd -- what a caller writes
without mmx_eval_skeleton_state_backward: the parameter transform (+ offsets), per joint the local transform
(translation = offset + t, rotation = preRot . Rz Ry Rx, scale = 2^sigma), then the world transforms composed level by level
(t = t_p + s_p R_p t_l, q = q_p (x) q_l, s = s_p s_l).  float64 on the CPU is the reference of the tests; the same code in
float32 is their yardstick, and on the device it is what scripts/state_backward_rate.py measures against.

channels_np / vjp_np: the numpy restatement of the channel formulas of momentum_amd/csrc/mmx_state_backward.hip with a DENSE
subtree sum, validated against the autograd gradient in tests/test_skeleton_state_reference.py (the way tests/tree_algebra_np.py
validates jt_times).  With a cotangent g = (g_t, g_q, g_s) on joint j and that joint's world state (t, q, s):
    F = g_t,   N = t x F + 1/2 Im(g_q (x) conj(q)),   D = t . F + s g_s
and for the joint-parameter row (a, dof) with the sums F_sub, N_sub, D_sub over the subtree of a (a included):
    translation   tau_d . F_sub                      tau_d = column d of s_p R_p (parent of a; identity for a root)
    rotation      omega . (N_sub - t_a x F_sub)      omega = the dof's world rotation axis
    scale         ln 2 (D_sub - t_a . F_sub)
"""
import numpy as np
import torch

LN2 = float(np.log(2.0))


def qmul(a, b):
    """Hamilton product, (x, y, z, w) storage."""
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack(
        [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz],
        -1,
    )


def qrot(q, v):
    u, w = q[..., :3], q[..., 3:]
    uv = 2.0 * torch.cross(u, v, dim=-1)
    return v + w * uv + torch.cross(u, uv, dim=-1)


def levels(parent):
    depth = np.zeros(len(parent), np.int64)
    for j, p in enumerate(parent):
        depth[j] = 0 if p < 0 else depth[p] + 1
    return [np.nonzero(depth == d)[0] for d in range(int(depth.max()) + 1)]


class RigTensors:
    """The rig's arrays as torch tensors of one dtype / device, and the level structure (built once per rig)."""

    def __init__(self, rig, dtype=torch.float64, device="cpu"):
        self.J, self.P = rig.num_joints, rig.num_params
        t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype, device=device)
        self.A = t(rig.dense_transform().astype(np.float64))  # [7J, P] (float32 entries, exactly)
        self.pt_offsets = t(rig.pt_offsets)
        self.offset = t(rig.translation_offset)
        self.pre = t(rig.pre_rotation)
        self.dtype, self.device = dtype, device
        lv = levels(rig.parent)
        order = np.concatenate(lv)  # joints in level order
        where = np.empty(self.J, np.int64)
        where[order] = np.arange(self.J)
        idx = lambda a: torch.as_tensor(np.asarray(a, np.int64), device=device)
        self.level_joints = [idx(l) for l in lv]
        self.level_parent_pos = [idx(where[rig.parent[l]]) for l in lv[1:]]  # the parents' places in level order
        self.to_joint_order = idx(where)


def skeleton_state(rt: RigTensors, theta, offset=None, pre=None):
    """theta [B, P] -> [B, J, 8] = (t, q (x, y, z, w), s); offset [B, J, 3] / pre [B, J, 4]: per-instance rig, else the rig's."""
    B = theta.shape[0]
    jp = (theta @ rt.A.T + rt.pt_offsets).reshape(B, rt.J, 7)
    off = rt.offset if offset is None else offset
    q0 = (rt.pre if pre is None else pre).expand(B, rt.J, 4)
    tl = off + jp[..., 0:3]
    h = 0.5 * jp[..., 3:6]
    s, c = torch.sin(h), torch.cos(h)
    z = torch.zeros_like(s[..., 0])
    qx = torch.stack([s[..., 0], z, z, c[..., 0]], -1)
    qy = torch.stack([z, s[..., 1], z, c[..., 1]], -1)
    qz = torch.stack([z, z, s[..., 2], c[..., 2]], -1)
    ql = qmul(qmul(qmul(q0, qz), qy), qx)
    sl = torch.exp2(jp[..., 6:7])
    l0 = rt.level_joints[0]
    t, q, sc = tl[:, l0], ql[:, l0], sl[:, l0]  # world transforms in level order, grown level by level
    for joints, ppos in zip(rt.level_joints[1:], rt.level_parent_pos):
        tp, qp, sp = t[:, ppos], q[:, ppos], sc[:, ppos]
        t = torch.cat([t, tp + qrot(qp, sp * tl[:, joints])], 1)
        q = torch.cat([q, qmul(qp, ql[:, joints])], 1)
        sc = torch.cat([sc, sp * sl[:, joints]], 1)
    return torch.cat([t, q, sc], -1)[:, rt.to_joint_order]


def vjp_autograd(rt: RigTensors, theta, cot, offset=None, pre=None):
    """d sum(cot * state) / d theta by torch autograd: theta [B, P], cot [B, J, 8] -> [B, P] (inputs as numpy or tensors)."""
    th = torch.as_tensor(np.asarray(theta), dtype=rt.dtype, device=rt.device).clone().requires_grad_(True)
    g = torch.as_tensor(np.asarray(cot), dtype=rt.dtype, device=rt.device)
    conv = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=rt.dtype, device=rt.device)
    (skeleton_state(rt, th, conv(offset), conv(pre)) * g).sum().backward()
    return th.grad.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatement of the kernel's formulas
# ---------------------------------------------------------------------------------------------------------------------------
def _qmul_np(a, b):
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])


def _qrot_np(q, v):
    uv = 2.0 * np.cross(q[:3], v)
    return v + q[3] * uv + np.cross(q[:3], uv)


def channels_np(state, g):
    """state [J, 8], g [J, 8] -> the seven channels F | N | D per joint [J, 7]."""
    out = np.zeros((state.shape[0], 7), state.dtype)
    for j in range(state.shape[0]):
        t, q, s = state[j, :3], state[j, 3:7], state[j, 7]
        F = g[j, :3]
        conj = np.concatenate([-q[:3], q[3:]])
        tau = 0.5 * _qmul_np(g[j, 3:7], conj)[:3]
        out[j, 0:3] = F
        out[j, 3:6] = np.cross(t, F) + tau
        out[j, 6] = t @ F + s * g[j, 7]
    return out


def axes_np(rig, theta, state, pre=None):
    """Per joint the translation axes (columns of s_p R_p) and the world rotation axes of rx, ry, rz: [J, 3, 3] each, column d."""
    J = rig.num_joints
    A = rig.dense_transform().astype(np.float64)
    jp = (A @ np.asarray(theta, np.float64) + rig.pt_offsets.astype(np.float64)).reshape(J, 7)
    pre = np.asarray(rig.pre_rotation if pre is None else pre, np.float64)
    tau, om = np.zeros((J, 3, 3)), np.zeros((J, 3, 3))
    e = np.eye(3)
    for j in range(J):
        p = int(rig.parent[j])
        qp = np.array([0.0, 0.0, 0.0, 1.0]) if p < 0 else state[p, 3:7]
        sp = 1.0 if p < 0 else state[p, 7]
        for d in range(3):
            tau[j][:, d] = sp * _qrot_np(qp, e[d])
        hz, hy = 0.5 * jp[j, 5], 0.5 * jp[j, 4]
        q0 = _qmul_np(qp, pre[j])
        q1 = _qmul_np(q0, np.array([0.0, 0.0, np.sin(hz), np.cos(hz)]))
        q2 = _qmul_np(q1, np.array([0.0, np.sin(hy), 0.0, np.cos(hy)]))
        om[j][:, 2] = _qrot_np(q0, e[2])
        om[j][:, 1] = _qrot_np(q1, e[1])
        om[j][:, 0] = _qrot_np(q2, e[0])
    return tau, om


def ancestor_or_self(parent):
    J = len(parent)
    anc = np.zeros((J, J))
    for j in range(J):
        a = j
        while a >= 0:
            anc[a, j] = 1.0
            a = int(parent[a])
    return anc


def vjp_np(rig, theta, state, g, pre=None):
    """The kernel's result for one instance from the channel formulas and a dense subtree sum: [P] (float64)."""
    state = np.asarray(state, np.float64)
    own = channels_np(state, np.asarray(g, np.float64))
    sub = ancestor_or_self(rig.parent) @ own  # [J, 7] sums over the subtree of each joint
    tau, om = axes_np(rig, theta, state, pre)
    out = np.zeros(rig.num_params)
    for r in range(7 * rig.num_joints):
        a, d = divmod(r, 7)
        Fs, Ns, Ds, ta = sub[a, 0:3], sub[a, 3:6], sub[a, 6], state[a, :3]
        if d < 3:
            v = tau[a][:, d] @ Fs
        elif d < 6:
            v = om[a][:, d - 3] @ (Ns - np.cross(ta, Fs))
        else:
            v = LN2 * (Ds - ta @ Fs)
        for k in range(rig.pt_outer[r], rig.pt_outer[r + 1]):
            out[rig.pt_inner[k]] += float(rig.pt_value[k]) * v
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# rigs and inputs of the tests
# ---------------------------------------------------------------------------------------------------------------------------
def make_rig(parent, triplets, num_params, seed=0, pt_offsets=False):
    """A rig over `parent` with random unit pre-rotations and offsets; triplets = (joint, dof, parameter, weight)."""
    from momentum_amd.rigs import _build_rig

    rng = np.random.default_rng(seed)
    J = len(parent)
    pre = rng.normal(size=(J, 4))
    pre /= np.linalg.norm(pre, axis=1, keepdims=True)
    off = rng.uniform(-1.0, 1.0, size=(J, 3))
    rig = _build_rig(parent, pre, off, [(7 * j + d, p, w) for j, d, p, w in triplets], num_params, [f"j{j}" for j in range(J)], [f"p{p}" for p in range(num_params)])
    if pt_offsets:
        rig.pt_offsets = rng.uniform(-0.2, 0.2, size=7 * J).astype(np.float32)
    return rig


def all_dofs_rig(parent, seed=0):
    """Every dof of every joint driven by a parameter of its own: P = 7 J."""
    J = len(parent)
    return make_rig(parent, [(j, d, 7 * j + d, 1.0) for j in range(J) for d in range(7)], 7 * J, seed)


def chain(J):
    return [-1] + list(range(J - 1))


def random_tree(J, seed):
    rng = np.random.default_rng(seed)
    return [-1] + [int(rng.integers(0, j)) for j in range(1, J)]


def table_rig(seed=5):
    """Table order and zero columns: parameter 0 drives three dofs on different joints with weights != 1; the rz of joint 2
    is driven by parameters 1 and 2; parameter 3 drives nothing; non-zero pt_offsets.  A five-joint tree with a branch."""
    parent = [-1, 0, 1, 1, 3]
    trip = [(1, 3, 0, 0.7), (3, 4, 0, -1.3), (4, 6, 0, 0.4), (2, 5, 1, 0.6), (2, 5, 2, -0.8), (0, 0, 4, 1.0), (0, 5, 5, 1.0), (4, 1, 6, 1.5), (0, 6, 7, 0.5)]
    return make_rig(parent, trip, 8, seed, pt_offsets=True)


def dof_kind(rig):
    """Per parameter the kind of dof it drives: 0 translation, 1 rotation, 2 scale (the kind of its first entry; -1: none)."""
    kind = np.full(rig.num_params, -1)
    for r in range(7 * rig.num_joints):
        for k in range(rig.pt_outer[r], rig.pt_outer[r + 1]):
            if kind[rig.pt_inner[k]] < 0:
                kind[rig.pt_inner[k]] = 0 if r % 7 < 3 else (1 if r % 7 < 6 else 2)
    return kind


def random_inputs(rig, B, seed):
    """Rotations uniform in +-1 rad, translations +-0.2, scales +-0.3; standard-normal cotangents on all eight channels."""
    rng = np.random.default_rng(seed)
    amp = np.array([0.2, 1.0, 0.3, 0.0])[dof_kind(rig)]
    theta = (rng.uniform(-1.0, 1.0, size=(B, rig.num_params)) * amp).astype(np.float32)
    cot = rng.normal(size=(B, rig.num_joints, 8)).astype(np.float32)
    return theta, cot
