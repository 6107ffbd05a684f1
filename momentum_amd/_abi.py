"""ctypes mirrors of the POD structs in include/mmx.h (the C-ABI boundary).

Pure plumbing: no compute here.  Field order and types must match include/mmx.h exactly;
tests/test_abi.py checks sizes and that the built library exports every declared symbol.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)

MMX_ABI_VERSION = 12
MMX_OK = 0
MMX_SOLVE_OK, MMX_SOLVE_NONFINITE, MMX_SOLVE_NOT_PD = 0, 1, 2
MMX_SOLVE_DAMPING_FLOORED = 4  # informational bit of status[] (include/mmx.h)
MMX_SOLVE_PRECISION_SUSPECT = 8  # informational: the single-precision solve's precision estimate exceeds options.precision_bound
MMX_SOLVE_ESCALATED_F64 = 16  # informational: MMX_PRECISION_AUTO re-solved the element in double
MMX_SOLVE_MIXED = 32  # informational: the element was solved by the mixed-precision instantiation (MMX_PRECISION_MIXED / AUTO)
MMX_SOLVE_ERROR_MASK = 3
MMX_PRECISION_F32, MMX_PRECISION_F64, MMX_PRECISION_AUTO, MMX_PRECISION_MIXED = 0, 1, 2, 3
MMX_MEM_HOST, MMX_MEM_DEVICE = 0, 1
MMX_LAYOUT_COL_MAJOR, MMX_LAYOUT_ROW_MAJOR = 0, 1
MMX_STEP_GN_FIXED_LAMBDA, MMX_STEP_LM_SCHEDULE, MMX_STEP_TRUST_REGION = 0, 1, 2


class RigDesc(C.Structure):
    _fields_ = [
        ("num_joints", C.c_int32),
        ("num_params", C.c_int32),
        ("parent", c_int32_p),
        ("pre_rotation", c_float_p),
        ("translation_offset", c_float_p),
        ("pt_outer", c_int32_p),
        ("pt_inner", c_int32_p),
        ("pt_value", c_float_p),
        ("pt_offsets", c_float_p),
    ]


class SkinDesc(C.Structure):
    """mmx_skin_desc: the skin of linear-blend skinning (host arrays)."""

    _fields_ = [
        ("num_vertices", C.c_int32),
        ("max_influences", C.c_int32),
        ("joint", c_int32_p),
        ("weight", c_float_p),
        ("inverse_bind", c_float_p),
        ("rest_positions", c_float_p),
    ]


MMX_MAX_SKIN_INFLUENCES = 8
# mmx_closest_points(batch, num_source, num_target, source, target, target_shared, source_normals, target_normals, max_dist,
# min_normal_dot, index, dist2, points, stream); mmx_closest_points_host: the same without the stream
CLOSEST_POINTS_ARGTYPES = (
    C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
)  # fmt: skip
# mmx_closest_points_plan(batch, num_source, num_target, with_normals, &sources_per_workgroup, &target_tile, &target_ways)
CLOSEST_POINTS_PLAN_ARGTYPES = (C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p)
# the vertex-normal entry points (include/mmx.h): name -> argument types, in the header's order
_MESH = (C.c_int32, C.c_int32, c_int32_p, C.c_int32)  # num_vertices, num_triangles, triangles (host), device
MESH_ARGTYPES = {
    "mmx_mesh_create": _MESH + (C.POINTER(C.c_void_p),),
    "mmx_mesh_destroy": (C.c_void_p,),
    "mmx_mesh_num_vertices": (C.c_void_p,),
    "mmx_mesh_num_triangles": (C.c_void_p,),
    "mmx_vertex_normals": (C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p),
    "mmx_vertex_normals_backward": (C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p),
    "mmx_vertex_normals_host": _MESH + (C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p),
    "mmx_vertex_normals_backward_host": _MESH + (C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p),
    "mmx_host_mesh_tables": (C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p),
}
# the closest-points-on-mesh entry points (include/mmx.h): name -> argument types, in the header's order
CLOSEST_POINTS_ON_MESH_ARGTYPES = {
    # (mesh, batch, num_source, source, vertices, vertices_shared, max_dist, face_index, barycentric, points, dist2, stream)
    "mmx_closest_points_on_mesh": (
        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
    ),
    # (the mesh itself, batch, num_source, source, vertices, vertices_shared, max_dist, face_index, barycentric, points, dist2)
    "mmx_closest_points_on_mesh_host": _MESH + (
        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
    ),
    # (batch, num_source, num_triangles, &sources_per_workgroup, &triangle_tile, &triangle_ways)
    "mmx_closest_points_on_mesh_plan": (C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p),
}  # fmt: skip
# vertex constraints on a skin (mmx_skin_normal_equations)
MMX_VC_POSITION, MMX_VC_PLANE = 0, 1
MMX_SKIN_NE_MAX_SOLVED = 128


class VertexConstraints(C.Structure):
    """mmx_vertex_constraints: the arrays of a batch of vertex constraints (device arrays, or host arrays for the _host form)."""

    _fields_ = [
        ("type", C.c_int32),
        ("count", C.c_int32),
        ("corners", C.c_int32),
        ("function_weight", C.c_float),
        ("vertex", C.c_void_p),
        ("barycentric", C.c_void_p),
        ("target", C.c_void_p),
        ("normal", C.c_void_p),
        ("weight", C.c_void_p),
        ("rest", C.c_void_p),
    ]


# (problem, skin, &constraints, theta, jtj, jtr, err, stream); the _host form: the same without the stream
SKIN_NORMAL_EQUATIONS_ARGTYPES = (
    C.c_void_p, C.c_void_p, C.POINTER(VertexConstraints), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
)  # fmt: skip
# the split form (an instance's tiles over several workgroups): name -> argument types, in the header's order
MMX_SKIN_NE_MAX_PARTS = 512
SKIN_NORMAL_EQUATIONS_SPLIT_ARGTYPES = {
    # (problem, skin, &constraints, theta, jtj, jtr, err, parts, workspace, workspace_bytes, stream)
    "mmx_skin_normal_equations_split": SKIN_NORMAL_EQUATIONS_ARGTYPES[:-1] + (C.c_int32, C.c_void_p, C.c_int64, C.c_void_p),
    # (problem, skin, &constraints, theta, jtj, jtr, err, parts)
    "mmx_skin_normal_equations_split_host": SKIN_NORMAL_EQUATIONS_ARGTYPES[:-1] + (C.c_int32,),
    # (batch, num_enabled, parts) -> int64
    "mmx_skin_normal_equations_workspace_bytes": (C.c_int32, C.c_int32, C.c_int32),
    # (batch, type, count, compute_units, workgroups_per_cu, &parts)
    "mmx_skin_normal_equations_plan": (C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p),
    # (problem, skin, &constraints, &parts)
    "mmx_skin_normal_equations_auto_parts": (C.c_void_p, C.c_void_p, C.POINTER(VertexConstraints), c_int32_p),
    # (tiles, parts, part, &begin, &end, &effective_parts)
    "mmx_skin_normal_equations_part_range": (C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p),
}
MMX_LOSS_WELSCH =float(np.finfo(np.float32).min)  # GeneralizedLossT::kWelsch
MMX_LIMIT_MINMAX = 0  # momentum::LimitType values (character/parameter_limits.h:20-31)
MMX_LIMIT_MINMAX_JOINT = 1
MMX_LIMIT_MINMAX_JOINT_PASSIVE = 2  # accepted and ignored, like LimitErrorFunctionT does
MMX_LIMIT_LINEAR = 3
MMX_LIMIT_LINEAR_JOINT = 4
MMX_LIMIT_HALFPLANE = 6


class ParameterLimit(C.Structure):
    """mmx_parameter_limit: one model-parameter entry of Character::parameterLimits."""

    _fields_ = [
        ("type", C.c_int32),
        ("index0", C.c_int32),
        ("index1", C.c_int32),
        ("weight", C.c_float),
        ("v", C.c_float * 4),
    ]

    @classmethod
    def minmax(cls, param, lo, hi, weight=1.0):
        return cls(MMX_LIMIT_MINMAX, int(param), 0, float(weight), (C.c_float * 4)(lo, hi, 0.0, 0.0))

    @classmethod
    def linear(cls, reference, target, scale, offset, range_min=0.0, range_max=0.0, weight=1.0):
        return cls(MMX_LIMIT_LINEAR, int(reference), int(target), float(weight), (C.c_float * 4)(scale, offset, range_min, range_max))

    @classmethod
    def minmax_joint(cls, joint, joint_parameter, lo, hi, weight=1.0):
        return cls(MMX_LIMIT_MINMAX_JOINT, 7 * int(joint) + int(joint_parameter), 0, float(weight), (C.c_float * 4)(lo, hi, 0.0, 0.0))

    @classmethod
    def minmax_joint_passive(cls, joint, joint_parameter, lo, hi, weight=1.0):
        return cls(MMX_LIMIT_MINMAX_JOINT_PASSIVE, 7 * int(joint) + int(joint_parameter), 0, float(weight), (C.c_float * 4)(lo, hi, 0.0, 0.0))

    @classmethod
    def linear_joint(cls, ref_joint, ref_parameter, tgt_joint, tgt_parameter, scale, offset, range_min=0.0, range_max=0.0, weight=1.0):
        return cls(MMX_LIMIT_LINEAR_JOINT, 7 * int(ref_joint) + int(ref_parameter), 7 * int(tgt_joint) + int(tgt_parameter),
                   float(weight), (C.c_float * 4)(scale, offset, range_min, range_max))  # fmt: skip

    @classmethod
    def halfplane(cls, param1, param2, n0, n1, offset, weight=1.0):
        return cls(MMX_LIMIT_HALFPLANE, int(param1), int(param2), float(weight), (C.c_float * 4)(n0, n1, offset, 0.0))


def limit_array(limits):
    """ctypes array (kept alive by the caller) of ParameterLimit."""
    arr = (ParameterLimit * max(len(limits), 1))()
    for i, l in enumerate(limits):
        arr[i] = l
    return arr


class EllipsoidLimit(C.Structure):
    """mmx_ellipsoid_limit: LimitType::Ellipsoid entry (character/parameter_limits.h:77-84)."""

    _fields_ = [
        ("ellipsoid", C.c_float * 12),
        ("ellipsoid_inv", C.c_float * 12),
        ("offset", C.c_float * 3),
        ("weight", C.c_float),
        ("ellipsoid_parent", C.c_int32),
        ("parent", C.c_int32),
    ]

    @classmethod
    def make(cls, parent, offset, ellipsoid_parent, translation, euler_zyx_deg, scale, weight=1.0):
        """The text form's arguments (parseEllipsoid, io/skeleton/parameter_limits_io.cpp:580-610):
        linear part = R(extrinsic XYZ of the reversed, radian angles) * diag(scale)."""
        ez = np.radians(np.asarray(euler_zyx_deg, np.float32).astype(np.float64))
        ax, ay, az = ez[2], ez[1], ez[0]
        cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
        R = np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                      [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                      [-sy, cy * sx, cy * cx]])  # Rz Ry Rx = eulerXYZToRotationMatrix(., Extrinsic), math/utility.cpp:315-380
        A = np.eye(4)
        A[:3, :3] = R @ np.diag(np.asarray(scale, np.float64))
        A[:3, 3] = np.asarray(translation, np.float64)
        return cls.from_affine(parent, offset, ellipsoid_parent, A[:3], weight)

    @classmethod
    def from_affine(cls, parent, offset, ellipsoid_parent, affine34, weight=1.0):
        A = np.eye(4)
        A[:3] = np.asarray(affine34, np.float64).reshape(3, 4)
        Ai = np.linalg.inv(A)
        f12 = lambda m: (C.c_float * 12)(*[float(x) for x in np.asarray(m[:3], np.float32).reshape(-1)])
        return cls(f12(A), f12(Ai), (C.c_float * 3)(*[float(x) for x in offset]), float(weight), int(ellipsoid_parent), int(parent))


def ellipsoid_array(items):
    arr = (EllipsoidLimit * max(len(items), 1))()
    for i, e in enumerate(items):
        arr[i] = e
    return arr


MMX_JC_PLANE, MMX_JC_HALF_PLANE, MMX_JC_AIM_DIST, MMX_JC_AIM_DIR = 0, 1, 2, 3
MMX_JC_FIXED_AXIS_DIFF, MMX_JC_FIXED_AXIS_COS, MMX_JC_FIXED_AXIS_ANGLE, MMX_JC_NORMAL = 4, 5, 6, 7
MMX_JC_PROJECTION, MMX_JC_DISTANCE = 8, 9  # ABI 12
MMX_JC_JOINT_TO_JOINT_DISTANCE = 10  # additive to ABI 12: the block's parent array holds the joints A, then the joints B
MMX_MAX_JOINT_BLOCKS = 8


def jc_func_dim(type_: int) -> int:
    """FuncDim of the block's error function (rows per constraint)."""
    if type_ in (MMX_JC_AIM_DIST, MMX_JC_AIM_DIR, MMX_JC_FIXED_AXIS_DIFF):
        return 3
    return 2 if type_ == MMX_JC_PROJECTION else 1


class JointConstraintBlock(C.Structure):
    """mmx_joint_constraint_block."""

    _fields_ = [
        ("type", C.c_int32),
        ("count", C.c_int32),
        ("parent", C.c_void_p),
        ("local_point", C.c_void_p),
        ("local_dir", C.c_void_p),
        ("global_", C.c_void_p),
        ("plane_d", C.c_void_p),
        ("weight", C.c_void_p),
        ("function_weight", C.c_float),
        ("loss_alpha", C.c_float),
        ("loss_c", C.c_float),
        # ABI 12
        ("projection", C.c_void_p),
        ("near_clip", C.c_float),
    ]


class JointBlock:
    """Python-side description of one further joint-constraint block (Plane / Aim / FixedAxis /
    Normal / Projection / Distance / JointToJointDistance error function).  Payload arrays are numpy ([K,..] for one
    instance or [B,K,..]) or, for the device path, contiguous float32 cuda tensors [B,K,..].  `projection` holds the
    projection block's 3 x 4 row-major camera matrices (12 floats per constraint).  `parent_b` ([K], the pair
    type only) is the second joint of every constraint; for that type `local_dir` is the offset on it (a point),
    `plane_d` the target distance and `global_` may be None."""

    FIELDS = (("local_point", 3), ("local_dir", 3), ("global_", 3), ("plane_d", 0), ("weight", 0), ("projection", 12))

    def __init__(self, type, parent, weight, global_, local_point=None, local_dir=None, plane_d=None,
                 function_weight: float = 1.0, loss=(2.0, 1.0), projection=None, near_clip: float = 1.0, parent_b=None):  # fmt: skip
        self.type = int(type)
        self.parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        self.count = int(self.parent.shape[0])
        self.parent_b = None if parent_b is None else np.ascontiguousarray(parent_b, dtype=np.int32).reshape(-1)
        if (self.type == MMX_JC_JOINT_TO_JOINT_DISTANCE) != (self.parent_b is not None):
            raise ValueError("parent_b goes with MMX_JC_JOINT_TO_JOINT_DISTANCE blocks, and only with them")
        if self.parent_b is not None and self.parent_b.shape[0] != self.count:
            raise ValueError(f"parent_b has {self.parent_b.shape[0]} joints for {self.count} constraints")
        self.weight, self.global_ = weight, global_
        self.local_point, self.local_dir, self.plane_d = local_point, local_dir, plane_d
        self.function_weight = float(function_weight)
        self.loss = (float(loss[0]), float(loss[1]))
        self.projection = projection
        self.near_clip = float(near_clip)

    @property
    def rows(self) -> int:
        return jc_func_dim(self.type) * self.count

    def instance(self, b: int) -> "JointBlock":
        def cut(a, d):
            if a is None:
                return None
            a = np.asarray(a, dtype=np.float32)
            shp = (-1, self.count, d) if d else (-1, self.count)
            return a.reshape(shp)[b]

        return JointBlock(self.type, self.parent, cut(self.weight, 0), cut(self.global_, 3), cut(self.local_point, 3),
                          cut(self.local_dir, 3), cut(self.plane_d, 0), self.function_weight, self.loss,
                          cut(self.projection, 12), self.near_clip, self.parent_b)  # fmt: skip

    def parent_array(self) -> np.ndarray:
        """What the C side reads as `parent`: [count], or [2 * count] (joints A, then joints B) for the pair type."""
        return self.parent if self.parent_b is None else np.ascontiguousarray(np.concatenate([self.parent, self.parent_b]))

    def struct(self, keep: list, batch=None, device: bool = False) -> JointConstraintBlock:
        """ctypes struct; arrays it points to are appended to `keep`.  batch = B checks [B,K,..] shapes."""
        ptrs = {}
        for name, d in self.FIELDS:
            a = getattr(self, name)
            if a is None:
                ptrs[name] = None
                continue
            if device:
                shp = (batch, self.count, d) if d else (batch, self.count)
                assert a.is_cuda and a.is_contiguous() and tuple(a.shape) == shp, (name, tuple(a.shape), shp)
                keep.append(a)
                ptrs[name] = C.c_void_p(a.data_ptr() if a.numel() else 0)
            else:
                x = np.ascontiguousarray(a, dtype=np.float32)
                if batch is not None:
                    x = x.reshape((batch, self.count, d) if d else (batch, self.count))
                keep.append(x)
                ptrs[name] = C.c_void_p(x.ctypes.data if x.size else 0)
        parents = self.parent_array()
        keep.append(parents)
        return JointConstraintBlock(
            self.type, self.count, C.c_void_p(parents.ctypes.data if self.count else 0), ptrs["local_point"], ptrs["local_dir"],
            ptrs["global_"], ptrs["plane_d"], ptrs["weight"], self.function_weight, self.loss[0], self.loss[1],
            ptrs["projection"], self.near_clip,
        )  # fmt: skip


def joint_block_array(blocks, keep: list, batch=None, device: bool = False):
    arr = (JointConstraintBlock * max(len(blocks), 1))()
    for i, blk in enumerate(blocks):
        arr[i] = blk.struct(keep, batch, device)
    return arr


class ConstraintData(C.Structure):
    _fields_ = [
        ("pos_offset", C.c_void_p),
        ("pos_target", C.c_void_p),
        ("pos_weight", C.c_void_p),
        ("ori_offset", C.c_void_p),
        ("ori_target", C.c_void_p),
        ("ori_weight", C.c_void_p),
        ("pos_function_weight", C.c_float),
        ("ori_function_weight", C.c_float),
        ("memory", C.c_int32),
        # optional parameter-space blocks
        ("model_target", C.c_void_p),
        ("model_weights", C.c_void_p),
        ("model_function_weight", C.c_float),
        ("num_limits", C.c_int32),
        ("limits", C.c_void_p),
        ("limit_function_weight", C.c_float),
        # GeneralizedLoss(alpha, c) of the position / orientation blocks; c <= 0 = default L2
        ("pos_loss_alpha", C.c_float),
        ("pos_loss_c", C.c_float),
        ("ori_loss_alpha", C.c_float),
        ("ori_loss_c", C.c_float),
        # further joint-constraint blocks (host array of JointConstraintBlock)
        ("num_joint_blocks", C.c_int32),
        ("joint_blocks", C.c_void_p),
        # Ellipsoid entries of the limit block (host array of EllipsoidLimit)
        ("num_ellipsoid_limits", C.c_int32),
        ("ellipsoid_limits", C.c_void_p),
        # per-element error-function weights [B][num_function_weights] (columns: position, orientation, limits, model, blocks...)
        ("function_weights", C.c_void_p),
        ("num_function_weights", C.c_int32),
    ]


class GnOptions(C.Structure):
    """POD mirror of SolverOptions + GaussNewtonSolverOptions
    (momentum/solver/solver.h:19-34, gauss_newton_solver.h:17-59)."""

    _fields_ = [
        ("min_iterations", C.c_int32),
        ("max_iterations", C.c_int32),
        ("threshold", C.c_float),
        ("regularization", C.c_float),
        ("do_line_search", C.c_int32),
        ("step_rule", C.c_int32),
        ("lm_lambda_min", C.c_float),
        ("lm_lambda_max", C.c_float),
        ("lm_up", C.c_float),
        ("lm_down", C.c_float),
        ("trust_region_radius", C.c_float),
        ("precision", C.c_int32),
        ("precision_bound", C.c_float),
    ]

    @classmethod
    def make(
        cls,
        min_iterations=1,
        max_iterations=2,
        threshold=1.0,
        regularization=0.05,
        do_line_search=False,
        step_rule=MMX_STEP_GN_FIXED_LAMBDA,
        lm_lambda_min=1e-6,
        lm_lambda_max=1e6,
        lm_up=4.0,
        lm_down=0.5,
        trust_region_radius=1.0,
        precision=MMX_PRECISION_F32,
        precision_bound=1e-5,
    ) -> "GnOptions":
        return cls(
            int(min_iterations),
            int(max_iterations),
            float(threshold),
            float(regularization),
            int(do_line_search),  # MMX_LINE_SEARCH_*: False/0 none, True/1 GaussNewtonSolverT rule, 2 SubsetGN / GN-QR rule
            int(step_rule),
            float(lm_lambda_min),
            float(lm_lambda_max),
            float(lm_up),
            float(lm_down),
            float(trust_region_radius),
            int(precision),
            float(precision_bound),
        )


ROUTES = {"auto": 0, "fused": 1, "wide": 2, "explicit_jacobian": 3, "wave": 4}  # MMX_ROUTE_*
# scope of the one-wavefront-per-instance route (MMX_WAVE_MAX_* in include/mmx.h)
WAVE_MAX_JOINTS = 64
WAVE_MAX_SOLVED = 32
WAVE_MAX_UNITS = 192


class Tuning(C.Structure):
    """mmx_tuning: which kernels mmx_solve runs (include/mmx.h)."""

    _fields_ = [("route", C.c_int32), ("max_refinement_steps", C.c_int32), ("mixed_tolerance", C.c_float), ("mixed_max_cg", C.c_int32), ("joint_pruning", C.c_int32), ("reserved", C.c_int32 * 3)]


def as_ptr(a: np.ndarray, ctype):
    """Typed pointer to a C-contiguous numpy array (caller keeps `a` alive)."""
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(C.POINTER(ctype))


def void_p(a) -> C.c_void_p:
    """void* of a numpy array, a raw device address (int) or None."""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(int(a))
