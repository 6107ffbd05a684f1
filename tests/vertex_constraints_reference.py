"""Reference of the vertex constraints' Gauss-Newton terms (mmx_skin_normal_equations; test infrastructure).

The scaled rows as a torch function of theta, composed from the two references that have their own checks --
skeleton_state_reference.skeleton_state and skinning_reference.skin_points --, parameterised by dtype:

    x_c = sum_{i < S} beta_ci out[b][v_ci]        out = skin_points(skeleton_state(theta))
    position  sigma_c (x_c - target_c)  (three rows)        plane  sigma_c n_c . (x_c - target_c)  (one row)
    sigma_c = sqrt(fw w_c)

A constraint whose weight is not > 0 (zero, negative, NaN) or with an index outside [0, V) in any corner is skipped: its rows
are exact zeros whatever its other arrays hold.  J by torch.autograd.functional.jacobian, then H = J[:, E]^T J[:, E],
g = J[:, E]^T r and err = |r|^2 over the enabled parameters E, ascending.  float64 on the CPU is the reference of the tests; the
same code in float32 is their yardstick.  Checked on its own in tests/test_vertex_constraints_reference.py.
"""
import numpy as np
import torch

from tests import skeleton_state_reference as fk
from tests import skinning_reference as skr


class Constraints:
    """The arrays of a batch of vertex constraints as numpy (float32 / int32 entries): target [B,C,3]; vertex None, [B,C] or
    [B,C,3]; barycentric None or [B,C,3]; normal None or [B,C,3] (plane type); weight None or [B,C]."""

    def __init__(self, target, vertex=None, barycentric=None, normal=None, weight=None, function_weight=1.0):
        self.target = np.asarray(target, np.float32)
        self.B, self.C = self.target.shape[:2]
        self.vertex = None if vertex is None else np.asarray(vertex, np.int32).reshape(self.B, self.C, -1)
        self.S = 1 if self.vertex is None else self.vertex.shape[2]
        self.barycentric = None if barycentric is None else np.asarray(barycentric, np.float32)
        self.normal = None if normal is None else np.asarray(normal, np.float32)
        self.weight = None if weight is None else np.asarray(weight, np.float32)
        self.fw = float(np.float32(function_weight))
        self.plane = self.normal is not None
        self.rows = self.C * (1 if self.plane else 3)

    def active(self, V):
        """[B, C] bool: the constraints that are not skipped."""
        ok = np.ones((self.B, self.C), bool)
        if self.weight is not None:
            with np.errstate(invalid="ignore"):
                ok &= self.weight > 0
        if self.vertex is not None:
            ok &= ((self.vertex >= 0) & (self.vertex < V)).all(-1)
        return ok

    def without_skipped(self, V):
        """The same constraints with every skipped one turned into a harmless zero-weight one on vertex 0 (finite arrays)."""
        act = self.active(V)
        z = lambda a, fill: None if a is None else np.where(act.reshape(act.shape + (1,) * (a.ndim - 2)), a, np.asarray(fill, a.dtype))
        w = np.where(act, np.ones_like(act, np.float32) if self.weight is None else np.nan_to_num(self.weight), 0).astype(np.float32)
        vertex = self.vertex if self.vertex is not None else np.broadcast_to(np.arange(self.C, dtype=np.int32)[None, :, None], (self.B, self.C, 1))
        return Constraints(z(self.target, 0), z(vertex, 0), z(self.barycentric, 0), z(self.normal, 0), w, self.fw)


def scaled_rows(rt: fk.RigTensors, sk: skr.SkinTensors, theta, con: Constraints, rest=None, offset=None, pre=None):
    """theta [B, P] (a tensor of rt.dtype) -> sigma f [B, rows]."""
    dt, dev = rt.dtype, rt.device
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dt, device=dev)
    B, C, S = con.B, con.C, con.S
    act = con.active(sk.V)
    out = skr.skin_points(sk, fk.skeleton_state(rt, theta, offset, pre), rest)  # [B, V, 3]
    vtx = np.broadcast_to(np.arange(C)[None, :, None], (B, C, 1)) if con.vertex is None else con.vertex
    vtx = np.where(act[..., None], vtx, 0).astype(np.int64)
    corners = out[torch.arange(B, device=dev)[:, None, None], torch.as_tensor(vtx, device=dev)]  # [B, C, S, 3]
    if con.barycentric is not None and S == 3:
        beta = t(np.where(act[..., None], con.barycentric, 0.0))
        x = (beta[..., None] * corners).sum(2)
    else:
        x = corners.sum(2)
    d = x - t(np.where(act[..., None], con.target, 0.0))
    w = np.ones((B, C), np.float32) if con.weight is None else con.weight
    sigma = torch.sqrt(t(np.float64(con.fw)) * t(np.where(act, w, 0.0)))
    if con.plane:
        f = (t(np.where(act[..., None], con.normal, 0.0)) * d).sum(-1)  # [B, C]
        r = sigma * f
    else:
        r = (sigma[..., None] * d).reshape(B, 3 * C)
    keep = torch.as_tensor(act if con.plane else np.repeat(act, 3, axis=1), device=dev)
    return torch.where(keep, r, torch.zeros((), dtype=dt, device=dev))


def jacobian(rt, sk, theta, con, rest=None, offset=None, pre=None):
    """(r [B, rows], J [B, rows, P]) by torch.autograd.functional.jacobian, instance by instance; theta numpy [B, P]."""
    th = torch.as_tensor(np.asarray(theta, np.float64), dtype=rt.dtype, device=rt.device)
    conv = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float64), dtype=rt.dtype, device=rt.device)
    rest, offset, pre = conv(rest), conv(offset), conv(pre)
    rs, Js = [], []
    for b in range(con.B):
        one = Constraints(
            con.target[b : b + 1], None if con.vertex is None else con.vertex[b : b + 1], None if con.barycentric is None else con.barycentric[b : b + 1],
            None if con.normal is None else con.normal[b : b + 1], None if con.weight is None else con.weight[b : b + 1], con.fw,
        )  # fmt: skip
        pick = lambda a: None if a is None else a[b : b + 1]
        f = lambda x: scaled_rows(rt, sk, x[None], one, pick(rest), pick(offset), pick(pre))[0]
        rs.append(f(th[b]).detach())
        # (one vectorised pass per parameter or per row, whichever is fewer: 128 against 900 on the humanoid's meshes)
        strategy = "forward-mode" if th.shape[1] < con.rows else "reverse-mode"
        Js.append(torch.autograd.functional.jacobian(f, th[b], vectorize=True, strategy=strategy))
    return torch.stack(rs).cpu().numpy(), torch.stack(Js).cpu().numpy()


def normal_equations(rig, skin, theta, con, enabled=None, rest=None, offset=None, pre=None, dtype=torch.float64):
    """dict(H [B, n, n], g [B, n], err [B], J [B, rows, n], r [B, rows]) as numpy arrays of `dtype`; skin = (joint, weight,
    inverse_bind, rest) arrays; enabled: None or a bool mask [P]."""
    rt = fk.RigTensors(rig, dtype)
    sk = skr.SkinTensors(skin[0], skin[1], skin[2], skin[3], rig.num_joints, dtype)
    r, J = jacobian(rt, sk, theta, con, rest, offset, pre)
    E = np.arange(rig.num_params) if enabled is None else np.nonzero(np.asarray(enabled))[0]
    J = J[:, :, E]
    return dict(H=np.einsum("bri,brj->bij", J, J), g=np.einsum("bri,br->bi", J, r), err=(r * r).sum(1), J=J, r=r)
