"""Host-side rig data model + synthetic rig generators.

`Rig` carries exactly what the hot path reads from a momentum::Character: the Skeleton
(parents, pre-rotations, translation offsets; momentum/character/joint.h:18-36,
skeleton.h:22-25) and the ParameterTransform as CSR (momentum/character/
parameter_transform.h:62-95).  Generators:

  make_test_character(n)   the reference's own fixture createTestCharacter(n)
                           (momentum/test/character/character_helpers.cpp:38-55,106-149)
  make_humanoid72(...)     BASELINE.json configs 2-4 (72-joint humanoid, P=128 or P=219)
  make_rig300(...)         BASELINE.json config 5 (300-joint hand+body rig, P=300)
  make_test_skin(...)      a synthetic skin (SkinWeights, inverse bind pose, rest vertices) on any of them

No compute lives here (integer/array bookkeeping only; make_test_skin composes the rest pose in float64 numpy to place
its vertices and invert the bind pose).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

from ._abi import RigDesc, as_ptr

PARAMS_PER_JOINT = 7  # momentum/character/types.h:21
TX, TY, TZ, RX, RY, RZ, SC = range(7)  # momentum/character/types.h:21-27


@dataclass
class Rig:
    """Skeleton + ParameterTransform (the two Character members the solver reads,
    momentum/character_solver/skeleton_solver_function.cpp:30-33)."""

    parent: np.ndarray  # [J] int32, -1 = kInvalidIndex
    pre_rotation: np.ndarray  # [J,4] float32 (x,y,z,w)
    translation_offset: np.ndarray  # [J,3] float32
    pt_outer: np.ndarray  # [7J+1] int32
    pt_inner: np.ndarray  # [nnz] int32
    pt_value: np.ndarray  # [nnz] float32
    pt_offsets: np.ndarray  # [7J] float32
    num_params: int
    joint_names: List[str] = field(default_factory=list)
    param_names: List[str] = field(default_factory=list)

    @property
    def num_joints(self) -> int:
        return int(self.parent.shape[0])

    def desc(self) -> RigDesc:
        """mmx_rig_desc pointing into this object's arrays (keep `self` alive)."""
        return RigDesc(
            self.num_joints,
            self.num_params,
            as_ptr(self.parent, C.c_int32),
            as_ptr(self.pre_rotation, C.c_float),
            as_ptr(self.translation_offset, C.c_float),
            as_ptr(self.pt_outer, C.c_int32),
            as_ptr(self.pt_inner, C.c_int32),
            as_ptr(self.pt_value, C.c_float),
            as_ptr(self.pt_offsets, C.c_float),
        )

    def depth(self) -> np.ndarray:
        d = np.zeros(self.num_joints, dtype=np.int32)
        for j in range(self.num_joints):
            p = int(self.parent[j])
            d[j] = 0 if p < 0 else d[p] + 1
        return d

    def dense_transform(self) -> np.ndarray:
        """7J x P dense copy of the parameter transform (tests only)."""
        A = np.zeros((PARAMS_PER_JOINT * self.num_joints, self.num_params), dtype=np.float32)
        for r in range(A.shape[0]):
            for k in range(self.pt_outer[r], self.pt_outer[r + 1]):
                A[r, self.pt_inner[k]] += self.pt_value[k]
        return A


def _build_rig(
    parent: Sequence[int],
    pre_rotation: np.ndarray,
    translation_offset: np.ndarray,
    triplets: Sequence[Tuple[int, int, float]],
    num_params: int,
    joint_names: List[str],
    param_names: List[str],
) -> Rig:
    """Triplets -> CSR with ascending columns per row (what Eigen's setFromTriplets yields,
    character_helpers.cpp:146)."""
    J = len(parent)
    rows = PARAMS_PER_JOINT * J
    parent = np.asarray(parent, dtype=np.int32)
    for j in range(J):  # Skeleton invariant parent < child (skeleton.cpp:16-22)
        assert parent[j] < j, "joints must be listed parent-before-child"
    acc: Dict[Tuple[int, int], float] = {}
    for r, c, v in triplets:
        assert 0 <= r < rows and 0 <= c < num_params
        acc[(r, c)] = acc.get((r, c), 0.0) + float(v)
    keys = sorted(acc.keys())
    outer = np.zeros(rows + 1, dtype=np.int32)
    for r, _ in keys:
        outer[r + 1] += 1
    outer = np.cumsum(outer).astype(np.int32)
    inner = np.array([c for _, c in keys], dtype=np.int32).reshape(-1)
    value = np.array([acc[k] for k in keys], dtype=np.float32).reshape(-1)
    return Rig(
        parent=parent,
        pre_rotation=np.ascontiguousarray(pre_rotation, dtype=np.float32),
        translation_offset=np.ascontiguousarray(translation_offset, dtype=np.float32),
        pt_outer=outer,
        pt_inner=inner,
        pt_value=value,
        pt_offsets=np.zeros(rows, dtype=np.float32),
        num_params=int(num_params),
        joint_names=list(joint_names),
        param_names=list(param_names),
    )


def make_test_character(num_joints: int = 3) -> Rig:
    """createTestCharacter(numJoints): straight chain, joint i offset UnitY, identity
    pre-rotations; parameters root_tx..root_rz, scale_global, joint1_rx, shared_rz (0.5 on
    joint1.rz and joint2.rz), jointK_rx for K >= 2
    (momentum/test/character/character_helpers.cpp:38-55,106-149)."""
    n = int(num_joints)
    assert n >= 3
    parent = [-1] + list(range(0, n - 1))
    pre = np.zeros((n, 4), dtype=np.float32)
    pre[:, 3] = 1.0
    off = np.zeros((n, 3), dtype=np.float32)
    off[1:, 1] = 1.0
    names = ["root_tx", "root_ty", "root_tz", "root_rx", "root_ry", "root_rz", "scale_global", "joint1_rx", "shared_rz"]
    rx_start = len(names)
    names += [f"joint{j}_rx" for j in range(2, n)]
    trip: List[Tuple[int, int, float]] = []
    for d in range(7):
        trip.append((0 * 7 + d, d, 1.0))
    trip.append((1 * 7 + RX, 7, 1.0))
    trip.append((1 * 7 + RZ, 8, 0.5))
    trip.append((2 * 7 + RZ, 8, 0.5))
    for j in range(2, n):
        trip.append((j * 7 + RX, rx_start + j - 2, 1.0))
    jn = ["root"] + [f"joint{i}" for i in range(1, n)]
    return _build_rig(parent, pre, off, trip, len(names), jn, names)


def _rand_quat_small(rng: np.random.Generator, max_angle: float) -> np.ndarray:
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    return np.array([*(np.sin(0.5 * ang) * axis), np.cos(0.5 * ang)], dtype=np.float32)


# joint table of the 72-joint humanoid: (name, parent name, limb axis used for the offset)
def _humanoid72_topology() -> List[Tuple[str, str, Tuple[float, float, float]]]:
    up, down, fwd = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0)
    t: List[Tuple[str, str, Tuple[float, float, float]]] = [("pelvis", "", (0.0, 0.0, 0.0))]
    prev = "pelvis"
    for n in ("spine1", "spine2", "spine3", "spine4", "neck", "head"):
        t.append((n, prev, up))
        prev = n
    t += [("jaw", "head", fwd), ("eye_l", "head", fwd), ("eye_r", "head", fwd)]
    for s, sx in (("l", 1.0), ("r", -1.0)):
        side = (sx, 0.0, 0.0)
        t.append((f"hip_{s}", "pelvis", side))
        t.append((f"knee_{s}", f"hip_{s}", down))
        t.append((f"ankle_{s}", f"knee_{s}", down))
        t.append((f"ball_{s}", f"ankle_{s}", fwd))
        t.append((f"toe_{s}", f"ball_{s}", fwd))
        t.append((f"toe_end_{s}", f"toe_{s}", fwd))
    for s, sx in (("l", 1.0), ("r", -1.0)):
        side = (sx, 0.0, 0.0)
        t.append((f"clavicle_{s}", "spine4", side))
        t.append((f"shoulder_{s}", f"clavicle_{s}", side))
        t.append((f"elbow_{s}", f"shoulder_{s}", side))
        t.append((f"forearm_twist_{s}", f"elbow_{s}", side))
        t.append((f"wrist_{s}", f"elbow_{s}", side))
        for f in ("thumb", "index", "middle", "ring", "pinky"):
            prevf = f"wrist_{s}"
            for k in range(4):
                nm = f"{f}{k}_{s}"
                t.append((nm, prevf, side))
                prevf = nm
    assert len(t) == 72
    return t


def make_humanoid72(seed: int = 12345, variant: str = "p128", unit: float = 1.0) -> Rig:
    """72-joint humanoid of BASELINE.json configs 2-4: pelvis root;
    spine 4 + neck + head + jaw/eyes 3; 2 x leg 6; 2 x (arm 4 + forearm twist 1 + 5 fingers x 4);
    depth 12.  Offsets U[2,30] (cm, times `unit`) along limb axes, pre-rotations random <= 0.3 rad.

    variant "p128": root 6 DOF + scale_global + rotations on articulated joints, a jaw
                    translation, finger curls shared across joints and three shared parameters
                    (fist_l, fist_r, spine_twist) like the fixture's shared_rz  -> P = 128
    variant "p219": 6 root DOF + 3 rotations on all 71 non-root joints      -> P = 219
    """
    rng = np.random.default_rng(seed)
    topo = _humanoid72_topology()
    names = [n for n, _, _ in topo]
    idx = {n: i for i, n in enumerate(names)}
    J = len(topo)
    parent = [-1 if p == "" else idx[p] for _, p, _ in topo]
    pre = np.zeros((J, 4), dtype=np.float32)
    off = np.zeros((J, 3), dtype=np.float32)
    for j, (_, p, axis) in enumerate(topo):
        pre[j] = _rand_quat_small(rng, 0.3) if j > 0 else np.array([0, 0, 0, 1], dtype=np.float32)
        if j > 0:
            length = rng.uniform(2.0, 30.0) * unit
            if topo[j][0].startswith(("thumb", "index", "middle", "ring", "pinky")):
                length = rng.uniform(2.0, 5.0) * unit  # finger segments
            a = np.asarray(axis, dtype=np.float64) + 0.15 * rng.normal(size=3)
            off[j] = (length * a / np.linalg.norm(a)).astype(np.float32)

    pnames: List[str] = []
    trip: List[Tuple[int, int, float]] = []

    def add_param(name: str, entries: Sequence[Tuple[str, int, float]]) -> None:
        col = len(pnames)
        pnames.append(name)
        for jn, dof, w in entries:
            trip.append((idx[jn] * 7 + dof, col, w))

    if variant == "p219":
        for d, nm in enumerate(("tx", "ty", "tz", "rx", "ry", "rz")):
            add_param(f"root_{nm}", [("pelvis", d, 1.0)])
        for n in names[1:]:
            for d, nm in ((RX, "rx"), (RY, "ry"), (RZ, "rz")):
                add_param(f"{n}_{nm}", [(n, d, 1.0)])
        assert len(pnames) == 219
    elif variant == "p128":
        for d, nm in enumerate(("tx", "ty", "tz", "rx", "ry", "rz")):
            add_param(f"root_{nm}", [("pelvis", d, 1.0)])
        add_param("scale_global", [("pelvis", SC, 1.0)])
        def rot3(n, dofs=((RX, "rx"), (RY, "ry"), (RZ, "rz"))):
            for d, nm in dofs:
                add_param(f"{n}_{nm}", [(n, d, 1.0)])

        # spine: rx/rz everywhere, ry individually on spine1/spine4 only; spine2/spine3 twist is
        # driven ONLY by the shared spine_twist parameter (no exactly-redundant parameters: a
        # redundant direction is a null space of J that fp32 noise / lambda drifts along)
        rot3("spine1")
        rot3("spine2", ((RX, "rx"), (RZ, "rz")))
        rot3("spine3", ((RX, "rx"), (RZ, "rz")))
        rot3("spine4")
        add_param("spine_twist", [("spine2", RY, 0.5), ("spine3", RY, 0.5)])
        for n in ("neck", "head", "jaw", "eye_l", "eye_r"):
            rot3(n)
        add_param("jaw_tz", [("jaw", TZ, 1.0)])  # a translation DOF below a non-root parent
        for s in ("l", "r"):
            for n in (f"hip_{s}", f"knee_{s}", f"ankle_{s}", f"ball_{s}", f"toe_{s}"):
                rot3(n)
        for s in ("l", "r"):
            for n in (f"clavicle_{s}", f"shoulder_{s}", f"elbow_{s}", f"wrist_{s}"):
                rot3(n)
            rot3(f"forearm_twist_{s}", ((RX, "rx"), (RY, "ry")))
        for s in ("l", "r"):
            for f in ("thumb", "index", "middle", "ring", "pinky"):
                dofs = ((RX, "rx"), (RY, "ry"), (RZ, "rz")) if f in ("thumb", "index") else ((RX, "rx"), (RZ, "rz"))
                rot3(f"{f}0_{s}", dofs)
                add_param(f"{f}_{s}_curl", [(f"{f}1_{s}", RZ, 0.6), (f"{f}2_{s}", RZ, 0.4)])
        for s in ("l", "r"):
            ent: List[Tuple[str, int, float]] = []
            for f in ("thumb", "index", "middle", "ring", "pinky"):
                ent += [(f"{f}0_{s}", RZ, 0.3), (f"{f}1_{s}", RZ, 0.2), (f"{f}2_{s}", RZ, 0.2)]
            add_param(f"fist_{s}", ent)
        assert len(pnames) == 128, len(pnames)
    else:
        raise ValueError(f"unknown variant {variant!r}")
    return _build_rig(parent, pre, off, trip, len(pnames), names, pnames)


# the 16 end-effector / landmark joints of BASELINE.json config 2
HUMANOID72_LANDMARKS = [
    "spine4", "head", "knee_l", "knee_r", "ankle_l", "ankle_r", "toe_l", "toe_r",
    "elbow_l", "elbow_r", "wrist_l", "wrist_r", "index3_l", "index3_r", "thumb3_l", "thumb3_r",
]  # fmt: skip


def humanoid72_landmark_joints(rig: Rig) -> np.ndarray:
    idx = {n: i for i, n in enumerate(rig.joint_names)}
    return np.array([idx[n] for n in HUMANOID72_LANDMARKS], dtype=np.int32)


def make_rig300(seed: int = 12345, unit: float = 1.0) -> Rig:
    """300-joint hand+body rig of BASELINE.json config 5: the 72-joint body plus 228 extra
    joints (dense hand / twist / leaf chains) attached by a seeded procedure, depth <= 16.
    Parameters: the 128 of the p128 body + one rotation on 172 of the extra joints -> P = 300."""
    base = make_humanoid72(seed, "p128", unit)
    rng = np.random.default_rng(seed + 1)
    J0 = base.num_joints
    parent = list(map(int, base.parent))
    names = list(base.joint_names)
    depth = list(map(int, base.depth()))
    pre = [base.pre_rotation[j] for j in range(J0)]
    off = [base.translation_offset[j] for j in range(J0)]
    while len(parent) < 300:
        # grow short chains off joints that still have depth head-room
        cand = [j for j in range(len(parent)) if depth[j] < 15]
        p = int(rng.choice(cand))
        chain = int(rng.integers(1, 4))
        for _ in range(chain):
            if len(parent) >= 300 or depth[p] >= 16:
                break
            j = len(parent)
            parent.append(p)
            depth.append(depth[p] + 1)
            names.append(f"extra{j}")
            pre.append(_rand_quat_small(rng, 0.3))
            a = rng.normal(size=3)
            off.append((rng.uniform(1.0, 8.0) * unit * a / np.linalg.norm(a)).astype(np.float32))
            p = j
    J = len(parent)
    assert J == 300 and max(depth) <= 16
    trip: List[Tuple[int, int, float]] = []
    for r in range(7 * J0):
        for k in range(base.pt_outer[r], base.pt_outer[r + 1]):
            trip.append((r, int(base.pt_inner[k]), float(base.pt_value[k])))
    pnames = list(base.param_names)
    extra = list(range(J0, J))
    chosen = sorted(rng.choice(extra, size=172, replace=False).tolist())
    for j in chosen:
        d = int(rng.integers(RX, RZ + 1))
        trip.append((j * 7 + d, len(pnames), 1.0))
        pnames.append(f"{names[j]}_r{'xyz'[d - RX]}")
    assert len(pnames) == 300
    return _build_rig(parent, np.stack(pre), np.stack(off), trip, len(pnames), names, pnames)


def rest_pose_transforms(rig: Rig) -> np.ndarray:
    """World transforms of the rest pose (all model parameters zero) as float64 3 x 4 affines [s R | t]: [J, 3, 4].  Array
    bookkeeping for make_test_skin (momentum/character/joint_state.cpp:22-65: local rotation = pre-rotation * rz * ry * rx)."""

    def qmul(a, b):
        av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
        return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])

    def qmat(q):
        x, y, z, w = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])  # fmt: skip

    J = rig.num_joints
    jp = rig.pt_offsets.astype(np.float64).reshape(J, PARAMS_PER_JOINT)
    out = np.zeros((J, 3, 4))
    quat, scale = np.zeros((J, 4)), np.ones(J)
    for j in range(J):
        q = rig.pre_rotation[j].astype(np.float64)
        for d, axis in ((RZ, 2), (RY, 1), (RX, 0)):
            h = np.zeros(4)
            h[axis], h[3] = np.sin(0.5 * jp[j, d]), np.cos(0.5 * jp[j, d])
            q = qmul(q, h)
        t, s = rig.translation_offset[j].astype(np.float64) + jp[j, :3], 2.0 ** jp[j, SC]
        p = int(rig.parent[j])
        if p >= 0:
            t = out[p, :, 3] + out[p, :, :3] @ t
            q, s = qmul(quat[p], q), scale[p] * s
        quat[j], scale[j] = q, s
        out[j, :, :3], out[j, :, 3] = s * qmat(q), t
    return out


@dataclass
class TestSkin:
    """A skin for Skin(rig_handle, joint, weight, inverse_bind, rest): what momentum's SkinWeights, Character::inverseBindPose
    and the mesh's rest vertices carry."""

    __test__ = False  # (not a pytest class)
    joint: np.ndarray  # [V,K] int32
    weight: np.ndarray  # [V,K] float32, rows sum to 1; unused slots 0
    inverse_bind: np.ndarray  # [J,12] float32, 3 x 4 row-major
    rest: np.ndarray  # [V,3] float32


def _bind_vertices(rig: Rig, pos: np.ndarray, children: List[List[int]], spread: float, rest: np.ndarray, K: int):
    """make_test_skin's weighting rule: (joint [V,K] int32, weight [V,K] float32) of rest positions [V,3] -- the nearest joint
    and its tree neighbours (parent, then children), weights 1 / (spread + distance) normalised to sum 1, unused slots weight
    0 on the nearest joint."""
    V = rest.shape[0]
    joint = np.zeros((V, K), np.int32)
    weight = np.zeros((V, K), np.float32)
    for v in range(V):
        near = int(np.argmin(np.linalg.norm(pos - rest[v], axis=1)))
        cand = [near] + ([int(rig.parent[near])] if rig.parent[near] >= 0 else []) + children[near]
        cand = cand[:K]
        w = 1.0 / (spread + np.linalg.norm(pos[cand] - rest[v], axis=1))
        w = (w / w.sum()).astype(np.float32)
        joint[v], joint[v, : len(cand)] = near, cand
        weight[v, : len(cand)] = w
    return joint, weight


def _inverse_bind(world: np.ndarray) -> np.ndarray:
    """Float64 inverses [J,3,4] of the 3 x 4 affines `world`."""
    J = world.shape[0]
    inv = np.zeros((J, 3, 4))
    for j in range(J):
        A = np.linalg.inv(world[j, :, :3])
        inv[j, :, :3], inv[j, :, 3] = A, -A @ world[j, :, 3]
    return inv


def _rig_neighbourhood(rig: Rig, pos: np.ndarray):
    """(children lists, spread = a quarter of the mean bone length) of a rig with rest-pose joint positions pos."""
    J = rig.num_joints
    children: List[List[int]] = [[] for _ in range(J)]
    for j in range(1, J):
        if rig.parent[j] >= 0:
            children[int(rig.parent[j])].append(j)
    bone = np.array([np.linalg.norm(pos[j] - pos[int(rig.parent[j])]) if rig.parent[j] >= 0 else 0.0 for j in range(J)])
    spread = 0.25 * (bone[bone > 0].mean() if (bone > 0).any() else 1.0)
    return children, spread


def make_test_skin(rig: Rig, num_vertices: int, max_influences: int, seed: int, random_affine: bool = False) -> TestSkin:
    """Synthetic skin for tests and scripts/skinning_rate.py: vertices scattered around the rest pose's bones, each bound to its
    nearest joint and that joint's tree neighbours (parent, then children) with positive weights that sum to 1; unused slots
    carry weight 0 (and the nearest joint's index).  inverse_bind is the float64 inverse of the rest-pose world transforms;
    random_affine perturbs every entry of it, so that the full 3 x 4 is exercised."""
    rng = np.random.default_rng(seed)
    J, V, K = rig.num_joints, int(num_vertices), int(max_influences)
    assert V >= 1 and 1 <= K <= 8
    world = rest_pose_transforms(rig)
    pos = world[:, :, 3]
    children, spread = _rig_neighbourhood(rig, pos)
    at = np.sort(rng.integers(0, J, size=V))  # bone by bone: neighbours in the vertex order share joints, as a mesh's do
    along = rng.uniform(0.0, 1.0, size=V)
    par = np.where(rig.parent[at] >= 0, rig.parent[at], at)
    rest = pos[at] + along[:, None] * (pos[par] - pos[at]) + spread * rng.normal(size=(V, 3))
    joint, weight = _bind_vertices(rig, pos, children, spread, rest, K)
    inv = _inverse_bind(world)
    if random_affine:
        inv += 0.1 * rng.normal(size=inv.shape)
    return TestSkin(joint, weight, inv.reshape(J, 12).astype(np.float32), rest.astype(np.float32))


@dataclass
class TestMesh:
    """A triangle mesh for capi.Mesh(triangles, num_vertices): positions [V,3] float32 and triangles [T,3] int32."""

    __test__ = False  # (not a pytest class)
    positions: np.ndarray
    triangles: np.ndarray


def make_test_mesh(nu: int, nv: int, noise: float, seed: int, offset=(0.0, 0.0, 0.0)) -> TestMesh:
    """Synthetic closed mesh for tests and scripts/vertex_normals_rate.py: a torus (major radius 0.3 around z, minor radius 0.1)
    as an nu x nv grid, vertex i * nv + j at major angle 2 pi i / nu and minor angle 2 pi j / nv, every quad split along the same
    diagonal into two outward-facing triangles: V = nu nv vertices of valence 6, T = 2 nu nv triangles.  Every coordinate is
    then jittered by a uniform draw from +-noise x the shortest grid edge, and `offset` is added."""
    nu, nv = int(nu), int(nv)
    assert nu >= 3 and nv >= 3
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    th, ph = 2.0 * np.pi * i.reshape(-1) / nu, 2.0 * np.pi * j.reshape(-1) / nv
    ring = 0.3 + 0.1 * np.cos(ph)
    pos = np.stack([ring * np.cos(th), ring * np.sin(th), 0.1 * np.sin(ph)], axis=1)
    at = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)
    v00, v10, v11, v01 = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
    tri = np.stack([np.stack([v00, v10, v11], axis=1), np.stack([v00, v11, v01], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    edges = np.concatenate([pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 1]], pos[tri[:, 0]] - pos[tri[:, 2]]])
    shortest = float(np.linalg.norm(edges, axis=1).min())
    pos = pos + float(noise) * shortest * rng.uniform(-1.0, 1.0, size=pos.shape) + np.asarray(offset, np.float64)
    return TestMesh(pos.astype(np.float32), tri)


def make_test_skinned_mesh(rig: Rig, nu: int, nv: int, max_influences: int, seed: int) -> Tuple[TestSkin, np.ndarray]:
    """(TestSkin, triangles [T,3] int32): the make_test_mesh torus (noise 0.1) bound to `rig` with make_test_skin's weighting
    rule.  The torus is scaled uniformly so that its diameter spans the longest side of the bounding box of the rest pose's
    joints and centred on that box."""
    K = int(max_influences)
    assert 1 <= K <= 8
    mesh = make_test_mesh(nu, nv, 0.1, seed)
    world = rest_pose_transforms(rig)
    pos = world[:, :, 3]
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    side = float((hi - lo).max())
    scale = (side if side > 0 else 1.0) / 0.8
    rest = 0.5 * (lo + hi) + scale * mesh.positions.astype(np.float64)
    children, spread = _rig_neighbourhood(rig, pos)
    joint, weight = _bind_vertices(rig, pos, children, spread, rest, K)
    inv = _inverse_bind(world)
    return TestSkin(joint, weight, inv.reshape(rig.num_joints, 12).astype(np.float32), rest.astype(np.float32)), mesh.triangles
