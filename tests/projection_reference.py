"""Double-precision reference for the projection and distance joint blocks (MMX_JC_PROJECTION / MMX_JC_DISTANCE,
include/mmx.h ABI 12), built on the CPU oracle's double results without teaching the oracle the new types.

The world point x = T_parent * offset of a constraint and its Jacobian dx/dtheta are the rows the oracle gives a
unit-weight L2 position constraint at the same parent and offset with target 0 (r = x, J = dx/dtheta).  The new rows are
df/dx . dx/dtheta in numpy float64, weighted like every joint block (rows sqrt(fw w) f, error fw w |f|^2), and are stacked
where the library puts them: after the position / orientation rows, before the limit / model-parameter rows."""
import numpy as np

from momentum_amd import _abi
from momentum_amd._abi import JointBlock
from oracle import oracle as orc


def world_points(rig, parents, offsets, theta):
    """x [K, 3] and dx/dtheta [K, 3, P] of the points `offsets` of joints `parents` (float64)."""
    parents = np.asarray(parents, np.int32).reshape(-1)
    K = len(parents)
    z = np.zeros
    cons = orc.Constraints(parents, np.asarray(offsets, np.float32).reshape(K, 3), z((K, 3)), np.ones(K), z(0, np.int32), z((0, 4)), z((0, 4)), z(0))
    J, r, _ = orc.eval_jacobian(rig, cons, np.asarray(theta, np.float64), dtype="f64")
    return r.reshape(K, 3), J.reshape(K, 3, -1)


def block_eval(blk: JointBlock, x):
    """f [K, d], df/dx [K, d, 3] and the clip mask [K] of one instance's block at world points x [K, 3]."""
    K = blk.count
    if blk.type == _abi.MMX_JC_PROJECTION:
        Pm = np.asarray(blk.projection, np.float32).astype(np.float64).reshape(K, 3, 4)
        A, a = Pm[:, :, :3], Pm[:, :, 3]
        p = np.einsum("kij,kj->ki", A, x) + a
        clipped = p[:, 2] < np.float64(np.float32(blk.near_clip))
        pz = np.where(clipped, 1.0, p[:, 2])
        u, v = p[:, 0] / pz, p[:, 1] / pz
        tgt = np.asarray(blk.global_, np.float32).astype(np.float64).reshape(K, 3)
        f = np.stack([u - tgt[:, 0], v - tgt[:, 1]], axis=1)
        d = np.stack([A[:, 0] - u[:, None] * A[:, 2], A[:, 1] - v[:, None] * A[:, 2]], axis=1) / pz[:, None, None]
        f[clipped] = 0.0
        d[clipped] = 0.0
        return f, d, clipped
    if blk.type == _abi.MMX_JC_DISTANCE:
        origin = np.asarray(blk.global_, np.float32).astype(np.float64).reshape(K, 3)
        diff = x - origin
        nrm = np.linalg.norm(diff, axis=1)
        f = (nrm - np.asarray(blk.plane_d, np.float32).astype(np.float64).reshape(K))[:, None]
        d = np.where(nrm[:, None] > 0, diff / np.where(nrm > 0, nrm, 1.0)[:, None], 0.0)[:, None, :]
        return f, d, np.zeros(K, bool)
    raise ValueError(f"not a projection / distance block: {blk.type}")


def block_rows(rig, blk: JointBlock, theta, fw_element: float = 1.0):
    """(J [rows, P], r [rows], error) of one instance's block at theta; fw_element = its per-element function weight."""
    x, dx = world_points(rig, blk.parent, blk.local_point, theta)
    f, d, _ = block_eval(blk, x)
    fw = np.float64(np.float32(blk.function_weight) * np.float32(fw_element))
    w = np.asarray(blk.weight, np.float32).astype(np.float64).reshape(-1)
    on = (w != 0) & (fw > 0)
    wgt = np.where(on, w * fw, 0.0)
    s = np.sqrt(np.maximum(wgt, 0.0))
    J = (s[:, None, None] * np.einsum("kdi,kip->kdp", d, dx)).reshape(-1, dx.shape[2])
    r = (s[:, None] * f).reshape(-1)
    return J, r, float(np.sum(wgt * np.sum(f * f, axis=1)))


def full_rows(rig, base, blocks, theta, fw_element=None):
    """J [M, P], r [M], error of one instance: the oracle's rows of `base` (an oracle Constraints WITHOUT joint blocks)
    with the rows of `blocks` (instance-sliced JointBlocks, projection / distance only) inserted after the position /
    orientation rows.  fw_element[i]: per-element function weight of block i (column 4 + i)."""
    J0, r0, e0 = orc.eval_jacobian(rig, base, np.asarray(theta, np.float64), dtype="f64")
    split = 3 * base.Kp + 9 * base.Ko
    Js, rs, err = [J0[:split]], [r0[:split]], e0
    for i, blk in enumerate(blocks):
        J, r, e = block_rows(rig, blk, theta, 1.0 if fw_element is None else fw_element[i])
        Js.append(J)
        rs.append(r)
        err += e
    Js.append(J0[split:])
    rs.append(r0[split:])
    return np.vstack(Js), np.concatenate(rs), err


def gauss_newton(rig, base, blocks, theta0, lam, iterations, enabled=None, fw_element=None):
    """Fixed-lambda Gauss-Newton in float64 (GaussNewtonSolverT's step: (J^T J + lambda I) delta = J^T r over the enabled
    columns, theta -= delta).  Returns theta after `iterations` steps.  lambda is rounded through float like
    mmx_gn_options::regularization."""
    lam = np.float64(np.float32(lam))
    th = np.asarray(theta0, np.float64).copy()
    E = np.arange(th.shape[0]) if enabled is None else np.flatnonzero(np.asarray(enabled))
    for _ in range(iterations):
        J, r, _ = full_rows(rig, base, blocks, th, fw_element)
        Jc = J[:, E]
        th[E] -= np.linalg.solve(Jc.T @ Jc + lam * np.eye(len(E)), Jc.T @ r)
    return th


def look_at_camera(eye, target, focal, up=(0.0, 1.0, 0.0)):
    """3 x 4 pinhole camera matrix K [R | -R eye] looking from `eye` at `target` (z forward, depth = distance along z)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    xa = np.cross(np.asarray(up, np.float64), z)
    xa /= np.linalg.norm(xa)
    ya = np.cross(z, xa)
    R = np.stack([xa, ya, z])
    Km = np.diag([focal, focal, 1.0])
    return Km @ np.hstack([R, (-R @ eye)[:, None]])


def random_cameras(rng, center, distance, focal, n):
    """n cameras on a ring around `center` at `distance`, slightly above or below it, looking at it."""
    cams = []
    for _ in range(n):
        ang = rng.uniform(0, 2 * np.pi)
        eye = np.asarray(center) + distance * np.array([np.sin(ang), rng.uniform(-0.3, 0.3), np.cos(ang)])
        cams.append(look_at_camera(eye, center, focal))
    return cams


def project(Pm, x):
    """(u, v) of world points x [K, 3] through 3 x 4 matrices Pm [K, 3, 4]."""
    p = np.einsum("kij,kj->ki", Pm[:, :, :3], x) + Pm[:, :, 3]
    return p[:, :2] / p[:, 2:3]


def keypoint_problem(rig, B, seed, pos_parents, proj_parents, n_cams=2, dist_parents=(), perturb=0.3, behind=False, near_clip=1.0,
                     distance=4.0):  # fmt: skip
    """Synthetic keypoint batch: element b has theta*_b = U[-perturb, perturb]^P (tests.helpers.make_problem, seed + b), position
    constraints on `pos_parents` with targets at theta*, the joints `proj_parents` seen by `n_cams` cameras around the
    character (targets = their projections at theta*, camera-major order) and distance constraints from random origins whose
    targets hold at theta*.  behind: one more projection constraint at the end, through a camera turned away (clipped).
    Returns (base oracle Constraints [B, ...] without joint blocks, [projection block, distance block (if any)] as batched
    JointBlocks, theta0 [B, P], theta* [B, P])."""
    from tests.helpers import make_problem

    base, th0, ths = make_problem(rig, pos_parents, [], B, seed=seed, perturb=perturb)
    pp = np.asarray(proj_parents, np.int32)
    dp = np.asarray(dist_parents, np.int32)
    parents = np.concatenate([np.tile(pp, n_cams), pp[:1]] if behind else [np.tile(pp, n_cams)]).astype(np.int32)
    K, Kd = len(parents), len(dp)
    proj = np.zeros((B, K, 12), np.float32)
    uv = np.zeros((B, K, 3), np.float32)
    origin = np.zeros((B, max(Kd, 1), 3), np.float32)
    dist = np.zeros((B, max(Kd, 1)), np.float32)
    for b in range(B):
        rng = np.random.default_rng(seed + 100003 + b)
        x, _ = world_points(rig, pp, np.zeros((len(pp), 3)), ths[b])
        center = x.mean(axis=0)
        cams = random_cameras(rng, center, distance, distance, n_cams)
        Pm = np.concatenate([np.repeat(c[None], len(pp), axis=0) for c in cams])
        if behind:
            away = cams[0] * np.array([[-1.0], [1.0], [-1.0]])  # turned by pi about its y axis: the character is behind it
            Pm = np.concatenate([Pm, away[None]])
        Pm = Pm.astype(np.float32)
        proj[b] = Pm.reshape(K, 12)
        xs, _ = world_points(rig, parents, np.zeros((K, 3)), ths[b])
        uv[b, :, :2] = project(Pm.astype(np.float64), xs)
        if Kd:
            xd, _ = world_points(rig, dp, np.zeros((Kd, 3)), ths[b])
            origin[b] = center + rng.uniform(-0.5, 0.5, size=(Kd, 3))
            dist[b] = np.linalg.norm(xd - origin[b].astype(np.float64), axis=1)
    zeros3 = np.zeros((B, K, 3), np.float32)
    blocks = [JointBlock(_abi.MMX_JC_PROJECTION, parents, np.ones((B, K), np.float32), uv, local_point=zeros3, projection=proj, near_clip=near_clip)]
    if Kd:
        blocks.append(JointBlock(_abi.MMX_JC_DISTANCE, dp, np.ones((B, Kd), np.float32), origin, local_point=np.zeros((B, Kd, 3), np.float32),
                                 plane_d=dist))  # fmt: skip
    return base, blocks, th0, ths
