/*
 * mmx.h -- C ABI of the MI355X-native batched inverse-kinematics hot path.
 *
 * This is the drop-in boundary for ONE path of facebookresearch/momentum: the
 * per-iteration  FK -> Jacobian/residual assembly -> (JtJ + lambda I) d = Jtr
 * -> theta update  loop, batched over independent characters.  Every entry point
 * cites the reference interface it replaces (paths relative to the reference
 * checkout).  Plain pointers and sizes only; no C++/torch types; status-code
 * returns, no exceptions across the ABI (the C++ shell in
 * include/momentum_amd/ converts non-zero into std::runtime_error to match
 * MT_CHECK/MT_THROW, momentum/common/checks.h:36-45, exception.h:24-66).
 *
 * Conventions shared with the reference:
 *   - quaternions are (x,y,z,w) (Eigen storage order; tensor API
 *     pymomentum/tensor_ik/tensor_error_function_utility.h:58-66),
 *   - joint parameter order per joint is tx,ty,tz,rx,ry,rz,scale
 *     (momentum/character/types.h:21-27, kParametersPerJoint = 7),
 *   - joints are listed parent-before-child (momentum/character/skeleton.cpp:16-22),
 *   - the dense Jacobian of one instance is COLUMN-MAJOR M x P
 *     (Eigen default; momentum/math/resizeable_matrix.h:18,32-34), rows ordered
 *     [position block (3 rows / constraint)] then [orientation block (9 rows /
 *     constraint)] = order of addErrorFunction
 *     (momentum/character_solver/skeleton_solver_function.cpp:217-261).
 *
 * Threading: one handle = one device + caller-provided stream; calls on one
 * handle must be serialised by the caller (the reference's solver objects are
 * not thread-safe either, momentum/math/resizeable_matrix.h:36-38).
 *
 * Streams and graphs: mmx_solve* / mmx_eval_* enqueue kernels and device-to-device
 * copies on `stream` and return; they neither wait for the stream nor read results
 * back (exceptions, each said at its declaration: the *_host conveniences, the
 * timed debug entry points, MMX_STEP_TRUST_REGION on the wide route).  After one
 * warm-up call on a handle (scratch buffers, LDS limits) such a call may therefore
 * be recorded into a HIP graph (hipStreamBeginCapture / torch.cuda.CUDAGraph) and
 * replayed on new values in the same buffers -- tests/test_gpu_graph.py; the
 * library issues kernel nodes only, no memset nodes.
 */
#ifndef MMX_H_
#define MMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMX_ABI_VERSION 12 /* 6: per-instance characters and constraint parents, MMX_STEP_TRUST_REGION (+ mmx_gn_options::
                             trust_region_radius), mmx_comm_* (RCCL), MMX_LIMIT_MINMAX_JOINT_PASSIVE, row-major J
                             7: mmx_tuning / mmx_problem_set_tuning / mmx_problem_last_route (replace the MMX_* environment
                             switches of earlier builds: the library reads no environment variable on the solve path)
                             8: columns in elimination order + tile-sparse factor on the wide route
                                (mmx_host_elimination_order, mmx_host_tile_structure, mmx_problem_tile_structure)
                             9: status[] is a bit set (MMX_SOLVE_DAMPING_FLOORED, informational), sized form of the
                                constraint call (mmx_problem_set_constraints_sized), mmx_eval_skeleton_state_host.
                             10: mmx_gn_options grows by `precision` / `precision_bound` (MMX_PRECISION_*: single, double, or
                                single with the elements whose precision estimate exceeds the bound re-solved in double),
                                status bits MMX_SOLVE_PRECISION_SUSPECT / MMX_SOLVE_ESCALATED_F64, MMX_SOLVE_FAILED(),
                                mmx_solve_with_step_history (damping and gain ratio per iteration of the LM schedule),
                                mmx_problem_solve_diagnostics.
                             11: MMX_PRECISION_MIXED (double forward kinematics / residuals / g = J^T r / linear-solve
                                residual around the single-precision factor: the double instantiation's answers at close to
                                the single-precision rate), which is also what MMX_PRECISION_AUTO now escalates to where it
                                applies; status bit MMX_SOLVE_MIXED; mmx_tuning grows mixed_tolerance / mixed_max_cg out of
                                its reserved words (same size).
                             12: joint-block types MMX_JC_PROJECTION (two rows) / MMX_JC_DISTANCE; mmx_joint_constraint_block
                                grows by `projection` / `near_clip` (the array stride of joint_blocks changes).
                             A caller MUST compare mmx_abi_version() with the MMX_ABI_VERSION it was compiled against
                             before any other call: the structs below grow at their end from version to version. */
#define MMX_PARAMS_PER_JOINT 7 /* momentum/character/types.h:21 */
#define MMX_INVALID_PARENT (-1) /* kInvalidIndex, momentum/character/types.h:182 */
#define MMX_MAX_MODEL_PARAMS 2048 /* kMaxModelParams, momentum/math/types.h:426 */

typedef enum mmx_status {
  MMX_OK = 0,
  MMX_ERR_INVALID_ARGUMENT = 1, /* MT_CHECK failure class */
  MMX_ERR_SIZE_MISMATCH = 2, /* solver.cpp:77, parameter_transform.cpp:112-121 */
  MMX_ERR_DEVICE = 3, /* HIP runtime error (message in mmx_last_error) */
  MMX_ERR_UNSUPPORTED = 4, /* shape outside what the kernels were built for */
  MMX_ERR_OUT_OF_MEMORY = 5,
  MMX_ERR_NO_DEVICE = 6 /* no gfx950 device: the product path never falls back to CPU */
} mmx_status;

/* Per-instance solve status (mmx_solve: status[B]). */
#define MMX_SOLVE_OK 0
#define MMX_SOLVE_NONFINITE 1 /* NaN/Inf result -> theta reverted to theta_init
                                 (pymomentum/tensor_ik/tensor_ik.cpp:168-173) */
#define MMX_SOLVE_NOT_PD 2 /* a Cholesky pivot came out non-positive in single precision (J rank deficient and
                              lambda below the rounding of J^T J).  Informational: a pivot at or below 2^-18 of its
                              row's H_jj + lambda drops that column from the iteration's step (zero step in that
                              parameter, the others solve the reduced system) and the step IS taken -- like the
                              reference, which never checks LLT::info() (gauss_newton_solver.cpp:251); its double
                              instantiation does not meet such pivots, its float instantiation hands Eigen's aborted
                              factor to solve().  The objective converges like the reference's; the components of
                              theta that J does not determine differ from the double solver's minimum-norm ones
                              (tests/test_gpu_weak_damping.py).  Since ABI 8 every single-precision
                              FACTOR is damped by at least 1e-5 of the mean diagonal of J^T J (the refinement measures
                              its residual with the caller's lambda through J, so the step is the caller's wherever J
                              determines it): the drop rule is the last resort and this status is rare. */

#define MMX_SOLVE_DAMPING_FLOORED 4 /* (bit, informational; since ABI 9 status[] is a bit set and MMX_SOLVE_NONFINITE /
                                       MMX_SOLVE_NOT_PD are its error bits, MMX_SOLVE_ERROR_MASK) in at least one
                                       iteration the caller's damping was below the floor of the single-precision
                                       FACTOR, 1e-5 of the mean diagonal of J^T J (the note above): what was factored is
                                       J^T J + floor I, the refinement pulled the step towards the caller's damping
                                       wherever J determines it, and the predicted decrease of the LM schedule / trust
                                       region was formed with the caller's value.  Where J is rank deficient or barely
                                       determined (BASELINE configs[0], configs[1] below lambda ~ 1e-3) such a solve
                                       is NOT within 1e-5 of the reference's double instantiation on the pose
                                       parameters -- no single-precision normal-equation solver is; the answer there
                                       is mmx_solve_f64.  mmx_solve_f64 never sets this bit. */
#define MMX_SOLVE_PRECISION_SUSPECT 8 /* (bit, informational, ABI 10) the single-precision solve's own estimate of its
                                         distance from the same solve in double -- 0.042 eps x max over the iterations of
                                         sqrt(error of the iteration / error of the first) / (smallest Cholesky pivot
                                         ratio d_jj / (H_jj + lambda) of the iteration) ~ eps x cond(J^T J + lambda I) x the
                                         residual's share (ABI 11; ABI 10 weighted every iteration with 1),
                                         calibrated as the 98th percentile of the relative distance on the BASELINE shapes;
                                         mmx_problem_solve_diagnostics returns it -- exceeds mmx_gn_options::precision_bound
                                         (default 1e-5, north_star's parity bound: 1 / ratio = 2000).  Unlike
                                         MMX_SOLVE_DAMPING_FLOORED, which only says that the factor's damping floor engaged,
                                         this follows the conditioning that loses the digits; it is a property of the problem
                                         class (rig, constraint set, lambda) more than of the instance: a class in which a
                                         few per cent of the instances leave the bound is marked as a whole.  With MMX_PRECISION_AUTO such elements (and the ones with an
                                         error bit) are solved again by the double instantiation from the initial parameters.
                                         One-launch and wide routes; the explicit-Jacobian route keeps
                                         MMX_SOLVE_DAMPING_FLOORED as its cue. */
#define MMX_SOLVE_ESCALATED_F64 16 /* (bit, informational, ABI 10) MMX_PRECISION_AUTO: this element's result comes from the
                                      double instantiation (its other status bits are that run's, plus the
                                      MMX_SOLVE_PRECISION_SUSPECT that sent it there) */
#define MMX_SOLVE_MIXED 32 /* (bit, informational, ABI 11) this element's result comes from the mixed-precision instantiation
                              (MMX_PRECISION_MIXED, or MMX_PRECISION_AUTO's second pass).  With it, MMX_SOLVE_PRECISION_SUSPECT
                              means that some iteration's conjugate gradients ran into mixed_max_cg before they met
                              mixed_tolerance (the single-precision factor was no preconditioner any more: cond x eps ~ 1). */
#define MMX_SOLVE_ERROR_MASK 3 /* (status & MMX_SOLVE_ERROR_MASK) == 0: the solve of that element is sound.  Mind the
                                  parentheses: in C `status & MMX_SOLVE_ERROR_MASK == 0` parses as status & (3 == 0). */
#define MMX_SOLVE_FAILED(status) (((status) & MMX_SOLVE_ERROR_MASK) != 0)

/* mmx_gn_options::precision (ABI 10). */
#define MMX_PRECISION_F32 0 /* the single-precision kernels (GaussNewtonSolverT<float>; what BASELINE's metric times) */
#define MMX_PRECISION_F64 1 /* mmx_solve with float parameters in and out, every element solved by the double instantiation
                               (GaussNewtonSolverT<double>, momentum/solver/gauss_newton_solver.cpp:315-316) */
#define MMX_PRECISION_AUTO 2 /* single precision first; the elements it marks MMX_SOLVE_PRECISION_SUSPECT (or whose solve
                                failed) are compacted and solved again in double from the initial parameters, on the same
                                stream, without a host round trip.  The batched driver's defaults (lambda = 0.01,
                                pymomentum/tensor_ik/solver_options.h:28-37) on marginally determined problems are where this
                                matters (profiles/r05_weak_damping.json).  ABI 11: the second pass is the
                                mixed-precision instantiation wherever that applies (MMX_SOLVE_MIXED instead of
                                MMX_SOLVE_ESCALATED_F64), and a problem class the FIRST factorisation already marks leaves the
                                single-precision pass at once (no ten iterations thrown away). */
#define MMX_PRECISION_MIXED 3 /* (ABI 11) one launch per solve like MMX_PRECISION_F32, with everything the answer's digits
                                 depend on in double: theta, forward kinematics, residual rows, g = J^T r and the residual of
                                 the linear solve -- all O(joints + constraints) tree passes -- while H = J^T J, its Cholesky
                                 factor and the triangular solves stay single precision and act as the preconditioner of a
                                 conjugate-gradient iteration whose operator is applied in double through the tree (classic
                                 mixed-precision iterative refinement; accurate while cond(J^T J + lambda I) x 6e-8 < 1).
                                 Follows GaussNewtonSolverT<double> (momentum/solver/gauss_newton_solver.cpp:315-316) to ~1e-7
                                 on theta -- at the batched driver's lambda = 0.01 and far below -- at a multiple of the double
                                 instantiation's rate.  Scope: the one-launch route's problems (up to 128 solved parameters,
                                 256 joints) with position / orientation constraints, limits on model / joint parameters and
                                 the model-parameter prior, every step rule but the trust region;
                                 anything else is solved by the double instantiation exactly as under MMX_PRECISION_F64 (no
                                 MMX_SOLVE_MIXED bit on the status). */

/* Where the caller's bulk arrays live. */
#define MMX_MEM_HOST 0
#define MMX_MEM_DEVICE 1

/* Jacobian layouts of mmx_eval_jacobian. */
#define MMX_LAYOUT_COL_MAJOR 0 /* J[b][p*M + i]   (the reference's layout) */
#define MMX_LAYOUT_ROW_MAJOR 1 /* J[b][i*P + p]   (torch-style [B][M][P]; assembled column-major, then transposed:
                                  one extra read + write of J; mmx_eval_jacobian[_host] only) */

/* Solver step rule. */
#define MMX_STEP_GN_FIXED_LAMBDA 0 /* GaussNewtonSolverT, constant regularization
                                      (momentum/solver/gauss_newton_solver.cpp:224-280) */
#define MMX_STEP_LM_SCHEDULE 1 /* gain-ratio lambda schedule, a lambda-form of
                                  momentum/character_solver/trust_region_qr.cpp:244-268
                                  (BASELINE configs[2]; no direct reference implementation) */
#define MMX_STEP_TRUST_REGION 2 /* TrustRegionQRT::doIteration (momentum/character_solver/trust_region_qr.cpp:
                                   52-270; LinearSolverType::TrustRegionQR of the batched driver, tensor_ik.cpp:
                                   150-152): per iteration up to ten trial steps, each after up to three Newton
                                   updates of the damping that pull |step| towards the trust radius (:180-231),
                                   gain ratio against the quadratic model (:246-247), radius x 0.25 / x 2 (cap 10)
                                   (:256-262), a step with rho <= 0 is rejected (:265-269).  Every change of the
                                   damping costs a factorisation (the reference appends rows to its QR).  Runs
                                   inside the one-launch solve where the problem fits it (<= 224 solved parameters,
                                   position / orientation constraints, limits, model prior) and on the wide route
                                   otherwise (driven from the host: factor / decide / trial kernels per trust step;
                                   larger systems, further joint error functions, ellipsoid limits); not on
                                   MMX_ROUTE_EXPLICIT_JACOBIAN.  mmx_solve_f64 runs the rule in double (one LL^T of
                                   J^T J + damping per value of the damping; 1e-7 on the oracle's double run where J
                                   has full column rank).  do_line_search and regularization are not read by this rule.
                                   DEVIATION from TrustRegionQRT: the reference's Householder QR of J takes the rule's
                                   (almost) zero damping on rank-deficient / under-determined J; an fp32 Cholesky of
                                   J^T J cannot, so the factor is damped by at least 1e-5 of the mean diagonal of J^T J
                                   (the refinement keeps the rule's damping): in the directions J does not determine
                                   the step is the more damped one -- the trust-region logic (radius, gain ratio,
                                   accept / reject) runs on that step; objective and iteration counts follow the
                                   oracle's on the reference's fixtures (tests/test_gpu_trust_region.py), the
                                   undetermined components of theta need not. */

/*
 * Static rig = Skeleton + ParameterTransform of a momentum::Character
 * (momentum/character/character.h:32-125; only .skeleton and
 * .parameterTransform are read on this path,
 * skeleton_solver_function.cpp:30-33).  All pointers are HOST pointers and are
 * copied by mmx_rig_create.
 */
typedef struct mmx_rig_desc {
  int32_t num_joints; /* J  = skeleton.joints.size() */
  int32_t num_params; /* P  = parameterTransform.numAllModelParameters() */
  const int32_t* parent; /* [J]  Joint::parent, -1 for kInvalidIndex (joint.h:18-36) */
  const float* pre_rotation; /* [J][4] Joint::preRotation (x,y,z,w) */
  const float* translation_offset; /* [J][3] Joint::translationOffset */
  /* ParameterTransform::transform, SparseRowMatrix 7J x P == CSR
     (momentum/character/parameter_transform.h:62-95, math/types.h:191) */
  const int32_t* pt_outer; /* [7J+1] outerIndexPtr */
  const int32_t* pt_inner; /* [nnz]  innerIndexPtr (column = model parameter) */
  const float* pt_value; /* [nnz]  valuePtr */
  const float* pt_offsets; /* [7J]   ParameterTransform::offsets (may be NULL = zeros) */
} mmx_rig_desc;

/*
 * Per-instance constraint payload = the std::vector<PositionDataT>/
 * <OrientationDataT> of one PositionErrorFunction + one OrientationErrorFunction
 * per batch element (momentum/character_solver/position_error_function.h:16-29,
 * orientation_error_function.h:16-36, error_function_types.h:34-44).  The parent
 * joint of each constraint is given at mmx_problem_create (batch-shared) or per
 * element with mmx_problem_set_instance_parents.  Orientation quaternions are normalised on ingest like the
 * OrientationDataT constructor does (orientation_error_function.h:33-35).
 */
/*
 * One entry of Character::parameterLimits restricted to the limit types that act on model or
 * joint PARAMETERS (momentum/character/parameter_limits.h:20-31,33-99,125-136): the rows of
 * LimitErrorFunctionT that need no joint transforms.  Ellipsoid limits travel in
 * mmx_ellipsoid_limit; the passive MinMaxJointPassive type is accepted and ignored like in the reference.
 */
#define MMX_LIMIT_MINMAX 0 /* LimitType::MinMax    : index0 = parameterIndex ; v = {min, max} */
#define MMX_LIMIT_MINMAX_JOINT 1 /* LimitType::MinMaxJoint : index0 = 7 * jointIndex + jointParameter (a row of the
                                    parameter transform) ; v = {min, max} on that JOINT parameter */
#define MMX_LIMIT_MINMAX_JOINT_PASSIVE 2 /* LimitType::MinMaxJointPassive: accepted and IGNORED -- LimitErrorFunctionT gives it
                                            neither an error term nor a Jacobian row (limit_error_function.cpp:836-837,
                                            1051-1052); such entries do not count in mmx_problem_num_rows */
#define MMX_LIMIT_LINEAR_JOINT 4 /* LimitType::LinearJoint : index0 = 7 * referenceJointIndex + referenceJointParameter,
                                    index1 = 7 * targetJointIndex + targetJointParameter ;
                                    v = {scale, offset, rangeMin, rangeMax} */
#define MMX_LIMIT_LINEAR 3 /* LimitType::Linear    : index0 = referenceIndex, index1 = targetIndex ;
                              v = {scale, offset, rangeMin, rangeMax}  (p_ref = scale * p_target - offset) */
#define MMX_LIMIT_HALFPLANE 6 /* LimitType::HalfPlane : index0 = param1, index1 = param2 ;
                                 v = {normal[0], normal[1], offset} */
#define MMX_LOSS_WELSCH (-3.402823466e+38f) /* GeneralizedLossT::kWelsch = numeric_limits<float>::lowest() */

typedef struct mmx_parameter_limit {
  int32_t type; /* MMX_LIMIT_* (values of momentum::LimitType) */
  int32_t index0;
  int32_t index1;
  float weight; /* ParameterLimit::weight */
  float v[4];
} mmx_parameter_limit;

/*
 * LimitType::Ellipsoid of Character::parameterLimits (momentum/character/parameter_limits.h:77-84):
 * the point `offset` of joint `parent` is pulled onto the ellipsoid (unit sphere mapped by `ellipsoid`)
 * defined in the frame of joint `ellipsoid_parent`.  Three rows per entry, evaluated like
 * computeEllipsoidError / computeEllipsoidJacobian (limit_error_function.cpp:173-195,702-790): the
 * Jacobian walks parent -> ellipsoid_parent (exclusive) and treats the projected point as constant,
 * weight kLimitWeight * weight_ * kPositionWeight(1e-4) * weight.  Affine maps are 3 x 4 row-major
 * [linear | translation].  Batch-shared, HOST array.  NB: no test of the reference exercises this
 * limit type, so parity for it rests on the restatement alone.
 */
typedef struct mmx_ellipsoid_limit {
  float ellipsoid[12]; /* LimitEllipsoid::ellipsoid */
  float ellipsoid_inv[12]; /* LimitEllipsoid::ellipsoidInv (its inverse) */
  float offset[3]; /* LimitEllipsoid::offset */
  float weight; /* ParameterLimit::weight */
  int32_t ellipsoid_parent;
  int32_t parent;
} mmx_ellipsoid_limit;

/*
 * The other JointErrorFunctionT specialisations: one block = one error
 * function object with `count` constraints per batch element.  FuncDim rows per constraint.
 *   type                      reference (momentum/character_solver/...)            rows  payload used
 *   MMX_JC_PLANE              PlaneErrorFunctionT(above=false) plane_error_function.cpp:52-71   1  local_point=offset, global=normal (normalised), plane_d
 *   MMX_JC_HALF_PLANE         PlaneErrorFunctionT(above=true)  (f clamped to <= 0, :63-70)      1  as above
 *   MMX_JC_AIM_DIST           AimDistErrorFunctionT aim_error_function.cpp:15-36                3  local_point, local_dir (normalised), global=globalTarget
 *   MMX_JC_AIM_DIR            AimDirErrorFunctionT  aim_error_function.cpp:39-67                3  as above
 *   MMX_JC_FIXED_AXIS_DIFF    FixedAxisDiffErrorFunctionT  fixed_axis_error_function.cpp:15-26  3  local_dir=localAxis, global=globalAxis (both normalised)
 *   MMX_JC_FIXED_AXIS_COS     FixedAxisCosErrorFunctionT   :28-39                               1  as above
 *   MMX_JC_FIXED_AXIS_ANGLE   FixedAxisAngleErrorFunctionT :41-66                               1  as above
 *   MMX_JC_NORMAL             NormalErrorFunctionT normal_error_function.cpp:14-31              1  local_point, local_dir=localNormal (normalised), global=globalPoint
 *   MMX_JC_PROJECTION         ProjectionErrorFunctionT (see the note below)                     2  local_point=offset, projection=P, global=(u, v, ignored), near_clip
 *   MMX_JC_DISTANCE           DistanceErrorFunctionT   (see the note below)                     1  local_point=offset, global=origin, plane_d=target distance
 *   MMX_JC_JOINT_TO_JOINT_DISTANCE  JointToJointDistanceErrorFunctionT (see the second note)    1  parent=[joints A | joints B], local_point=offset on A,
 *                                                                                                  local_dir=offset on B (a point), plane_d=target distance
 * Vectors are normalised on ingest exactly where the reference's data constructors do
 * (plane_error_function.h:30, aim_error_function.h:34, fixed_axis_error_function.h:29-30,
 * normal_error_function.h:34).
 *
 * The two point functions of ABI 12, with x = T_parent * offset (the point of a position constraint, t + s R o):
 *   MMX_JC_PROJECTION  p = A x + a with P = [A | a] (3 x 4 row-major, [B][count][12]).  p.z < near_clip: the constraint is
 *                      skipped (no error, rows zero).  Otherwise f = (p.x / p.z - u, p.y / p.z - v),
 *                      df/dx = (1 / p.z) [A_0 - (p.x / p.z) A_2 ; A_1 - (p.y / p.z) A_2] (A_i: row i of A).
 *   MMX_JC_DISTANCE    f = |x - origin| - d, df/dx = (x - origin)^T / |x - origin| (zero where the norm is zero).
 * Both are weighted like every block above (error fw * w * |f|^2, rows sqrt(fw * w) f) and take the L2 loss only: a block of
 * either type with another loss (loss_c > 0 and (alpha, c) != (2, 1)) is refused with MMX_ERR_UNSUPPORTED.
 * PROVENANCE: these restate momentum's ProjectionErrorFunctionT (ProjectionConstraintDataT: projection, parent, offset,
 * weight, target; constructor argument nearClip, default 1) and DistanceErrorFunctionT (DistanceConstraintDataT: origin,
 * target, parent, offset, weight) from memory of the reference, without a checkout at hand, so they carry no file:line
 * citations yet.  To confirm against the reference: the near-clip test p.z < nearClip and its default of 1; that neither
 * function applies a constant weight factor (like kPositionWeight); that neither takes a robust loss.
 *
 * The pair function (additive to ABI 12: no struct grows, the version stays), the first that ties two joints to each other
 * instead of one joint to the world.  With x_a = T_A * offset_a and x_b = T_B * offset_b (each the point of a position constraint):
 *   MMX_JC_JOINT_TO_JOINT_DISTANCE  f = |x_a - x_b| - d, df/dx_a = n^T, df/dx_b = -n^T with n = (x_a - x_b) / |x_a - x_b|
 *                      (both zero where the norm is zero: the row is zero and the residual -sqrt(fw w) d, as for MMX_JC_DISTANCE).
 *                      Row: sqrt(fw w) n^T (dx_a/dtheta - dx_b/dtheta); it walks the ancestor chains of BOTH joints and cancels
 *                      on their common part.  Error fw * w * f^2.
 *   `parent` holds 2 * count joints for this type alone: the `count` joints A, then the `count` joints B (A = B and A an
 *   ancestor of B are legal).  `local_dir` is the offset on B, a point: it is NOT normalised on ingest.  `global`,
 *   `projection` and `near_clip` are not read (`global` may be NULL).  L2 loss only, refused like the two types above.
 * PROVENANCE: this restates momentum's JointToJointDistanceErrorFunctionT (constraint data: joint1, offset1, joint2, offset2,
 * targetDistance, weight) from memory of the reference, without a checkout at hand, so it carries no file:line citations yet.
 * To confirm against the reference: that the function applies no constant weight factor (like kPositionWeight); that it
 * takes no robust loss; what it does at zero distance (here: zero row, residual -sqrt(fw w) d).
 */
#define MMX_JC_PLANE 0
#define MMX_JC_HALF_PLANE 1
#define MMX_JC_AIM_DIST 2
#define MMX_JC_AIM_DIR 3
#define MMX_JC_FIXED_AXIS_DIFF 4
#define MMX_JC_FIXED_AXIS_COS 5
#define MMX_JC_FIXED_AXIS_ANGLE 6
#define MMX_JC_NORMAL 7
#define MMX_JC_PROJECTION 8 /* ABI 12 */
#define MMX_JC_DISTANCE 9 /* ABI 12 */
#define MMX_JC_JOINT_TO_JOINT_DISTANCE 10 /* additive to ABI 12: parent is [2 * count] */
#define MMX_MAX_JOINT_BLOCKS 8

typedef struct mmx_joint_constraint_block {
  int32_t type; /* MMX_JC_* */
  int32_t count; /* constraints per batch element */
  const int32_t* parent; /* [count] HOST, batch-shared: ConstraintData::parent (MMX_JC_JOINT_TO_JOINT_DISTANCE: [2 * count], joints A then joints B) */
  const float* local_point; /* [B][count][3] or NULL when the type has no point */
  const float* local_dir; /* [B][count][3] or NULL when the type has no direction (MMX_JC_JOINT_TO_JOINT_DISTANCE: the offset on joint B) */
  const float* global; /* [B][count][3] (MMX_JC_JOINT_TO_JOINT_DISTANCE: not read, may be NULL) */
  const float* plane_d; /* [B][count] (plane types; MMX_JC_DISTANCE / MMX_JC_JOINT_TO_JOINT_DISTANCE: the target distance) */
  const float* weight; /* [B][count] ConstraintData::weight */
  float function_weight; /* SkeletonErrorFunction::weight_ */
  float loss_alpha, loss_c; /* GeneralizedLossT(alpha, c); c <= 0: default L2, c = 1 */
  /* ---- ABI 12 */
  const float* projection; /* [B][count][12] MMX_JC_PROJECTION only: 3 x 4 row-major camera matrix, same memory kind */
  float near_clip; /* MMX_JC_PROJECTION only: constraints with p.z < near_clip are skipped (must be finite) */
} mmx_joint_constraint_block;

typedef struct mmx_constraint_data {
  const float* pos_offset; /* [B][Kp][3] */
  const float* pos_target; /* [B][Kp][3] */
  const float* pos_weight; /* [B][Kp]    ConstraintData::weight */
  const float* ori_offset; /* [B][Ko][4] (x,y,z,w) */
  const float* ori_target; /* [B][Ko][4] (x,y,z,w) */
  const float* ori_weight; /* [B][Ko] */
  float pos_function_weight; /* SkeletonErrorFunction::weight_ of the position block
                                (skeleton_error_function.h:44-141, setWeight) */
  float ori_function_weight; /* ... of the orientation block */
  int32_t memory; /* MMX_MEM_HOST: copied; MMX_MEM_DEVICE: borrowed, caller keeps alive */
  /* ---- optional parameter-space blocks (all zero / NULL = absent); rows follow the
     orientation rows: [3 Kp][9 Ko][num_limits][P if model_target != NULL] */
  /* ModelParametersErrorFunctionT::setTargetParameters (model_parameters_error_function.h:48-51) */
  const float* model_target; /* [B][P] targetParameters_, same memory kind as above */
  const float* model_weights; /* [B][P] targetWeights_ */
  float model_function_weight; /* weight_ of that block */
  /* LimitErrorFunctionT::setLimits (limit_error_function.h:88-89): batch-shared, ALWAYS a host
     pointer (copied) */
  int32_t num_limits;
  const mmx_parameter_limit* limits; /* [num_limits] */
  float limit_function_weight; /* weight_ of that block */
  /* ---- robust loss of the two joint-constraint blocks: GeneralizedLossT(alpha, c)
     (momentum/math/generalized_loss.h:46-101; constructor arguments lossAlpha / lossC of
     PositionErrorFunctionT / OrientationErrorFunctionT, position_error_function.h:41-48).
     alpha = 2: L2, 1: L1 / pseudo-Huber, 0: Cauchy, MMX_LOSS_WELSCH: Welsch, other: Barron's
     general form.  c <= 0 (e.g. a zero-initialised struct) selects the default L2 loss with c = 1. */
  float pos_loss_alpha, pos_loss_c;
  float ori_loss_alpha, ori_loss_c;
  /* ---- optional further joint-constraint blocks (see mmx_joint_constraint_block); their rows
     follow the orientation rows and precede the limit rows:
     [3 Kp][9 Ko][block 0]...[block n-1][num_limits][P if model_target != NULL].
     `joint_blocks` is a HOST array (copied); the payload arrays inside follow `memory`.
     Problems with such blocks are solved by the explicit-Jacobian kernels. */
  int32_t num_joint_blocks; /* <= MMX_MAX_JOINT_BLOCKS */
  const mmx_joint_constraint_block* joint_blocks;
  /* ---- Ellipsoid entries of the limit block (same weight_ = limit_function_weight as `limits`);
     three rows each, placed between the joint-block rows and the other limit rows:
     [3 Kp][9 Ko][blocks][3 num_ellipsoid_limits][num_limits][P].  HOST array (copied). */
  int32_t num_ellipsoid_limits;
  const mmx_ellipsoid_limit* ellipsoid_limits;
  /* ---- per-element error-function weights = errorFunctionWeights[iBatch][weightsMap[iErr]] of the batched driver
     (pymomentum/tensor_ik/tensor_ik.cpp:100-101,137-138; tensor_ik_utility.cpp:162-177: every error function of
     element iBatch gets setWeight(that entry)).  NULL = none.  [B][num_function_weights] floats, same memory kind as
     the constraint arrays (device: borrowed), columns:
        0 position block   1 orientation block   2 limit block (parameter + ellipsoid limits)
        3 model-parameter block   4 + i joint block i        (columns past num_function_weights count as 1)
     Element b's weight_ of a block = the block's scalar function weight above x function_weights[b][column]; the
     driver's weights go here with the scalars left at 1.  A product <= 0 switches the block off for that element
     (skeleton_solver_function.cpp:223-231), like weightsMap[iErr] < 0 does (weight 0, tensor_ik_utility.cpp:176). */
  const float* function_weights;
  int32_t num_function_weights;
} mmx_constraint_data;

/*
 * POD mirror of SolverOptions + GaussNewtonSolverOptions
 * (momentum/solver/solver.h:19-34, gauss_newton_solver.h:17-59).
 */
/*
 * Backtracking rules of the reference's Gauss-Newton solvers (tau = 0.5, at most 10 trial steps, the
 * last trial stays when none passes):
 *   MMX_LINE_SEARCH_GAUSS_NEWTON  GaussNewtonSolverT::updateParameters (gauss_newton_solver.cpp:283-313):
 *                                 accept when  e - e(alpha) >= alpha * 1e-3 * e
 *   MMX_LINE_SEARCH_DIRECTIONAL   SubsetGaussNewtonSolverT::doIteration (subset_gauss_newton_solver.cpp:
 *                                 117-142) and GaussNewtonSolverQRT::doIteration (gauss_newton_solver_qr.cpp:
 *                                 126-149) -- the two solvers the batched driver builds
 *                                 (pymomentum/tensor_ik/tensor_ik.cpp:142-158): accept when
 *                                 e - e(alpha) >= 1e-4 * alpha * (J^T r . delta)
 */
#define MMX_LINE_SEARCH_NONE 0
#define MMX_LINE_SEARCH_GAUSS_NEWTON 1
#define MMX_LINE_SEARCH_DIRECTIONAL 2

typedef struct mmx_gn_options {
  int32_t min_iterations; /* SolverOptions::minIterations (default 1) */
  int32_t max_iterations; /* SolverOptions::maxIterations (default 2) */
  float threshold; /* SolverOptions::threshold (default 1): converged when
                      |e_prev-e|/(|e|+FLT_MIN) <= threshold*FLT_EPSILON, solver.cpp:98-99 */
  float regularization; /* GaussNewtonSolverBaseOptions::regularization (default 0.05) */
  int32_t do_line_search; /* MMX_LINE_SEARCH_* (default 0 = GaussNewtonSolverBaseOptions::doLineSearch false) */
  int32_t step_rule; /* MMX_STEP_* */
  /* LM schedule knobs (only read when step_rule == MMX_STEP_LM_SCHEDULE) */
  float lm_lambda_min; /* default 1e-6 */
  float lm_lambda_max; /* default 1e6 */
  float lm_up; /* lambda *= lm_up   when rho < 0.25 or the step is rejected (default 4) */
  float lm_down; /* lambda *= lm_down when rho > 0.75 (default 0.5) */
  /* trust region (only read when step_rule == MMX_STEP_TRUST_REGION) */
  float trust_region_radius; /* TrustRegionQROptions::trustRegionRadius_ (default 1; <= 0 selects the default) */
  /* ABI 10 */
  int32_t precision; /* MMX_PRECISION_* (default MMX_PRECISION_F32); read by mmx_solve / mmx_solve_with_history /
                        mmx_solve_with_step_history / mmx_solve_host, not by mmx_solve_f64 */
  float precision_bound; /* estimate above which an element is MMX_SOLVE_PRECISION_SUSPECT (default 1e-5; <= 0 selects the
                            default) */
} mmx_gn_options;

typedef struct mmx_rig mmx_rig; /* opaque: device-resident rig constants */
typedef struct mmx_problem mmx_problem; /* opaque: one batch of B instances on one device */

/* Sensible defaults == the reference's struct initialisers cited above. */
void mmx_gn_options_default(mmx_gn_options* opt);

/* ABI / build info. */
int32_t mmx_abi_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* mmx_last_error(void);
/* Number of visible HIP devices (0 when there is none; never throws). */
int32_t mmx_device_count(void);

/*
 * Replaces: constructing Skeleton + ParameterTransform for
 * SkeletonSolverFunctionT (skeleton_solver_function.cpp:25-39).  Validates the
 * parent-before-child invariant (skeleton.cpp:16-22) and CSR bounds, uploads the
 * rig and its derived integer tables to `device`.
 */
int32_t mmx_rig_create(const mmx_rig_desc* desc, int32_t device, mmx_rig** out);
void mmx_rig_destroy(mmx_rig* rig);
int32_t mmx_rig_num_joints(const mmx_rig* rig);
int32_t mmx_rig_num_params(const mmx_rig* rig);

/*
 * Replaces: one SkeletonSolverFunctionT + PositionErrorFunctionT +
 * OrientationErrorFunctionT per batch element, as built per task in
 * pymomentum/tensor_ik/tensor_ik.cpp:136-141.  pos_parent / ori_parent are HOST
 * arrays of joint indices (ConstraintData::parent).  All device scratch is sized
 * here, once.
 */
int32_t mmx_problem_create(
    mmx_rig* rig,
    int32_t batch,
    int32_t num_pos,
    const int32_t* pos_parent,
    int32_t num_ori,
    const int32_t* ori_parent,
    mmx_problem** out);
void mmx_problem_destroy(mmx_problem* problem);

/*
 * Per-instance characters of the same topology: the batched driver solves element iBatch on
 * *characters[iBatch] (pymomentum/tensor_ik/tensor_ik.cpp:129,140), in practice one skeleton scaled per
 * subject -- same parents and parameter transform, different Joint::translationOffset / preRotation.
 * translation_offset [B][J][3], pre_rotation [B][J][4] (x,y,z,w); either may be NULL (= the rig's own
 * values for every element); both NULL restores the shared rig.  `memory`: MMX_MEM_HOST (copied) or
 * MMX_MEM_DEVICE (borrowed, caller keeps alive).  Every entry point of the problem (FK, J assembly,
 * solve) then reads element b's constants.
 */
int32_t mmx_problem_set_instance_rig(
    mmx_problem* problem,
    const float* translation_offset,
    const float* pre_rotation,
    int32_t memory,
    void* stream);

/*
 * Per-instance constraint parents: ConstraintData::parent of element iBatch's constraint k, the way the
 * tensor error functions read `parents` per batch element (pymomentum/tensor_ik/
 * tensor_marker_error_function.cpp:97-98,186).  pos_parent [B][Kp], ori_parent [B][Ko] (joint indices);
 * either may be NULL (= the batch-shared list given at mmx_problem_create); both NULL restores the
 * shared lists.  `memory` as above.  The integer bookkeeping that depends on where constraints sit
 * (structurally zero columns, the solve list) is rebuilt for the UNION of the batch's parents -- a column
 * that is zero for one element only gets an exact zero step there, as in the reference.
 * Joint indices are validated (MT_CHECK joint_error_function-inl.h:230).
 */
int32_t mmx_problem_set_instance_parents(
    mmx_problem* problem,
    const int32_t* pos_parent,
    const int32_t* ori_parent,
    int32_t memory,
    void* stream);

/*
 * Which kernels mmx_solve runs.  The library picks by problem size (MMX_ROUTE_AUTO); a caller -- in practice a parity
 * test that wants every route exercised on the same inputs, or a benchmark -- can pin the route per problem handle.
 * A pinned route the problem does not fit makes mmx_solve return MMX_ERR_UNSUPPORTED; it never falls through silently.
 *   MMX_ROUTE_FUSED              one launch, one workgroup per instance, the system in LDS (<= 224 solved parameters)
 *   MMX_ROUTE_WIDE               normal equations from the tree moments, left-looking blocked Cholesky over the
 *                                structurally non-zero 16 x 16 tiles (columns in elimination order) -- the factor resident
 *                                in LDS while its tiles fit half a CU (<= ~75 tiles), in HBM beyond --, refinement through
 *                                the tree (<= 512 solved parameters; the default from 129 on)
 *   MMX_ROUTE_EXPLICIT_JACOBIAN  dense J in HBM -> J^T J (matrix cores; VALU beyond 384 columns) -> Cholesky step; the route
 *                                for problems outside the tree kernels' scope, among them systems of 513 ... 2048 solved
 *                                parameters (kMaxModelParams, momentum/math/types.h:426-429: a rig cannot have more)
 *   MMX_ROUTE_WAVE               one launch, ONE WAVEFRONT per instance (four instances per workgroup, no workgroup barrier in
 *                                the iteration loop), the system in registers and a few KB of LDS: the route for small rigs.
 *                                MMX_ROUTE_AUTO never picks it yet; it is taken only when pinned (and by mmx_solve_frames, which
 *                                runs on it: one wavefront per SEQUENCE of frames).  Scope (anything else, pinned,
 *                                is MMX_ERR_UNSUPPORTED with a message that names the condition, before theta or any output is
 *                                touched):
 *                                  rig          <= MMX_WAVE_MAX_JOINTS joints, any tree shape, any parameter count, per-instance
 *                                               offsets / pre-rotations (mmx_problem_set_instance_rig)
 *                                  system       1 .. MMX_WAVE_MAX_SOLVED solved parameters after the enabled mask and the
 *                                               structural-zero elimination (shared parameters and every dof kind included)
 *                                  constraints  position + orientation blocks with the L2 loss, at most MMX_WAVE_MAX_UNITS
 *                                               constraint vectors (positions + 3 x orientations), constraint / block / per-element
 *                                               function weights (columns 0 and 1); NOT robust losses, further joint blocks,
 *                                               ellipsoid or parameter limits, the model-parameter prior, per-instance parents
 *                                  options      MMX_STEP_GN_FIXED_LAMBDA, every do_line_search rule, MMX_PRECISION_F32; NOT the
 *                                               LM schedule, the trust region, MMX_PRECISION_F64 / AUTO / MIXED
 *                                  outputs      final_error, iterations, status, error and parameter history;
 *                                               mmx_problem_solve_diagnostics after such a solve answers MMX_ERR_UNSUPPORTED and
 *                                               MMX_SOLVE_PRECISION_SUSPECT is never set
 *                                Added without an ABI bump (one enum value, no struct grows): a library that predates the route
 *                                answers mmx_problem_set_tuning with MMX_ERR_INVALID_ARGUMENT -- that is the feature probe.
 * The route does not change WHAT is computed (same algorithm, same refinement); results of different routes agree to
 * rounding (tests/test_gpu_weak_damping.py, tests/test_gpu_fuzz.py).
 */
#define MMX_ROUTE_AUTO 0
#define MMX_ROUTE_FUSED 1
#define MMX_ROUTE_WIDE 2
#define MMX_ROUTE_EXPLICIT_JACOBIAN 3
#define MMX_ROUTE_WAVE 4
#define MMX_WAVE_MAX_JOINTS 64
#define MMX_WAVE_MAX_SOLVED 32
#define MMX_WAVE_MAX_UNITS 192 /* keeps a wave's share of LDS under 16 KB at 64 joints */
typedef struct mmx_tuning {
  int32_t route; /* MMX_ROUTE_* */
  int32_t max_refinement_steps; /* iterative-refinement steps a solve may take per iteration on top of the fp32 Cholesky
                                   solve (each measures its residual through J itself): 0 = the default, up to three (a
                                   further one only while the last correction exceeded 1e-3 of the step); 1..3 = at most
                                   that many; -1 = none (a measurement switch: north_star's 1e-5 needs the refinement) */
  float mixed_tolerance; /* (ABI 11) MMX_PRECISION_MIXED: the conjugate gradients of an iteration stop when the predicted size of
                            the next correction falls below this fraction of the step (0 = the default, 3e-9: north_star's 1e-5
                            then holds on every element whose double run amplifies a 1e-12 perturbation by less than 1e5; 1e-7
                            costs 15 % less and holds it where the amplification stays below 1e2) */
  int32_t mixed_max_cg; /* ... and after at most this many operator applications (0 = the default, 12) */
  int32_t joint_pruning; /* (out of the reserved words, same size; no ABI bump: a library that predates it answers -1 with
                            MMX_ERR_INVALID_ARGUMENT) 0 = the default, on: the one-launch solve, its mixed-precision
                            instantiation, the wave route and the wide route's tree kernels run over the LIVE joints only --
                            the ancestors-or-self of every joint the problem references (constraint parents, both joints of
                            the further blocks and of ellipsoid limits, the joints of joint-parameter limits), renumbered by
                            monotone maps.  A joint outside that set has no constraint below it: its columns are structurally
                            zero and nothing the solve returns reads its state, so results are BIT-IDENTICAL either way
                            (tests/test_gpu_live_joints.py).  -1 = off (a measurement switch, like max_refinement_steps = -1).
                            Nothing is pruned with per-instance rigs or constraint parents, when every joint is live or when
                            none is referenced.  Routes, instantiations and LDS budgets are chosen from the full joint count
                            in both settings. */
  int32_t reserved[3]; /* must be zero */
} mmx_tuning;
int32_t mmx_problem_set_tuning(mmx_problem* problem, const mmx_tuning* tuning);
/* MMX_ROUTE_* the last mmx_solve / mmx_solve_with_history on this handle took (MMX_ROUTE_AUTO before the first). */
int32_t mmx_problem_last_route(const mmx_problem* problem);
/* The joint count the solve kernels named under mmx_tuning::joint_pruning run over with the problem's current tables and
 * tuning: the live joints, or mmx_rig_num_joints when nothing is pruned.  (Additive, host-side query.) */
int32_t mmx_problem_num_solve_joints(const mmx_problem* problem);
/* Which form of the double kernel mmx_solve_f64 (MMX_PRECISION_F64, the last stage of MMX_PRECISION_AUTO) would launch for the
 * problem's current tables: *resident = 1 when packed H and a chunk of J stay in LDS, 0 for the form that keeps J and H in the
 * problem's global scratch; *chunk_rows = the rows of J that form assembles per chunk.  Either output may be null.  No GPU
 * work, no allocation.  MMX_ERR_UNSUPPORTED where mmx_solve_f64 would refuse the rig (beyond the kernel's LDS budget).
 * (Additive, host-side query.) */
int32_t mmx_problem_f64_form(const mmx_problem* problem, int32_t* resident, int32_t* chunk_rows);

/* M = 3*Kp + 9*Ko + rows of the further blocks and parameter-space blocks
 * (JointErrorFunctionT::getJacobianSize, joint_error_function-inl.h:300-302). */
int32_t mmx_problem_num_rows(const mmx_problem* problem);
int32_t mmx_problem_batch(const mmx_problem* problem);

/*
 * Replaces SolverT::setEnabledParameters -> SkeletonSolverFunctionT::
 * setEnabledParameters (solver.cpp:40-47, skeleton_solver_function.cpp:45-61):
 * enabled[P] (HOST, 0/1) is the ParameterSet; derives activeJointParams
 * (parameter_transform.cpp:97-107) and the compacted enabled list
 * (gauss_newton_solver.cpp:57-66).  Default after create: all enabled.
 */
int32_t mmx_problem_set_enabled(mmx_problem* problem, const uint8_t* enabled);

/* Replaces PositionErrorFunctionT::setConstraints / OrientationErrorFunctionT::
 * setConstraints + setWeight for every batch element. */
int32_t mmx_problem_set_constraints(
    mmx_problem* problem,
    const mmx_constraint_data* data,
    void* stream);
/* The same with sizeof(mmx_constraint_data) AS THE CALLER WAS COMPILED: mmx_constraint_data grows at its end (ABI 8
 * appended function_weights / num_function_weights), and a caller built against an older header hands over a shorter
 * struct.  Fields past data_size read as zero / NULL (= absent); a data_size larger than this library's struct is
 * MMX_ERR_INVALID_ARGUMENT (the caller is newer than the library).  Bindings should call this form
 * (the C++ shell and the ctypes plumbing do); mmx_problem_set_constraints trusts the full current layout. */
int32_t mmx_problem_set_constraints_sized(
    mmx_problem* problem,
    const mmx_constraint_data* data,
    size_t data_size,
    void* stream);

/*
 * The graded kernel and the parity hook.  Replaces, per batch element,
 * SkeletonSolverFunctionT::initializeJacobianComputation + computeJacobianBlock
 * for both blocks (skeleton_solver_function.cpp:200-261 ->
 * joint_error_function-inl.h:179-297) into a pre-zeroed dense Jacobian
 * (gauss_newton_solver.cpp:166).  theta_dev [B][P], jac_dev [B][M*P] in `layout`,
 * res_dev [B][M], err_dev [B] (double, may be NULL) are DEVICE pointers.
 * Every element of jac_dev is written (zeros included).
 */
int32_t mmx_eval_jacobian(
    mmx_problem* problem,
    const float* theta_dev,
    float* jac_dev,
    float* res_dev,
    double* err_dev,
    int32_t layout,
    void* stream);

/*
 * Profiling aid: mmx_eval_jacobian with a pair of HIP events attached to the dispatch packet of the
 * J-assembly kernel itself (hipExtLaunchKernelGGL): *kernel_ms receives the duration of that kernel
 * on `stream`, without launch latency or the gap to neighbouring dispatches -- the quantity a
 * rocprofv3 kernel trace reports.  Synchronises the stream.  bench.py's roofline uses it.
 */
int32_t mmx_eval_jacobian_timed(
    mmx_problem* problem,
    const float* theta_dev,
    float* jac_dev,
    float* res_dev,
    double* err_dev,
    int32_t layout,
    void* stream,
    float* kernel_ms);

/*
 * Profiling aid: the store pattern of the J-assembly kernel on its own -- every element of
 * jac_dev [B][M*P] is written with the same stores, workgroup shape and column-major layout, but no
 * kinematics.  *kernel_ms = duration of that kernel (events on its dispatch packet).  The bandwidth
 * it reaches is what the write pattern allows on the box at hand; bench.py reports it next to the
 * J-assembly figure (roofline.store_pattern_gbs).  Problems with position / orientation rows only.
 */
int32_t mmx_debug_store_pattern(mmx_problem* problem, float* jac_dev, void* stream, float* kernel_ms);

/*
 * Forward pass only.  Replaces SkeletonStateT<T>(params, skeleton)
 * (skeleton_state.cpp:22-28,87-121).  state_dev [B][J][8] =
 * (tx,ty,tz, qx,qy,qz,qw, s) world transforms (the layout of
 * pymomentum's skel_state tensors).
 */
int32_t mmx_eval_skeleton_state(
    mmx_problem* problem,
    const float* theta_dev,
    float* state_dev,
    void* stream);

/*
 * Normal equations of one GN step without solving them: H = J[:,E]^T J[:,E]
 * (full symmetric n x n, n = |E| enabled parameters, row-major == col-major),
 * g = J[:,E]^T r.  Replaces GaussNewtonSolverT::computeJtJFromJacobianBlocks
 * (gauss_newton_solver.cpp:110-221).  jtj_dev [B][n*n], jtr_dev [B][n].
 */
int32_t mmx_eval_normal_equations(
    mmx_problem* problem,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    double* err_dev,
    void* stream);

/*
 * Replaces, for every batch element, SolverT::solve with a GaussNewtonSolverT
 * (solver.cpp:50-128, gauss_newton_solver.cpp:224-313) exactly as the batched
 * driver does per task (tensor_ik.cpp:127-177), including its NaN/Inf revert.
 * theta_dev [B][P] in/out (DEVICE).  Optional DEVICE outputs (NULL to skip):
 *   final_error[B]   double  the value solve() returns (error at the theta
 *                            before the last step, solver.cpp:126-127)
 *   iterations[B]    int32   errorHistory_.size()
 *   status[B]        int32   MMX_SOLVE_* (a bit set; MMX_SOLVE_FAILED(status[b]) tests the error bits)
 *   error_history    double [B][max_iterations] (unused tail = 0)
 */
int32_t mmx_solve(
    mmx_problem* problem,
    const mmx_gn_options* options,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    void* stream);

/*
 * The double instantiation: SolverT<double>::solve with GaussNewtonSolverT<double> for every element
 * (momentum/solver/gauss_newton_solver.cpp:315-316; solveTensorIKProblem is templated on T,
 * pymomentum/tensor_ik/tensor_ik.cpp:95-103).  theta_dev is DOUBLE [B][P]; the constraint payload and the joint
 * constants stay float (Joint is float in the reference even for double solves, skeleton_state.cpp:89) and are
 * widened per use; every other argument as in mmx_solve.  Normal equations from the explicit Jacobian, LL^T and
 * two substitutions in double: agrees with the reference's double solver to rounding (tests: 1e-10 against the
 * oracle), no refinement step.  Built for exactness, not for the roofline: position / orientation
 * constraints and the further joint error functions (mmx_joint_constraint_block) with their losses, parameter limits
 * incl. ellipsoid limits, the model-parameter prior, per-element error-function weights, per-instance characters and
 * parents, fixed lambda, the LM schedule or the trust region (MMX_STEP_TRUST_REGION), both line-search rules.
 */
int32_t mmx_solve_f64(
    mmx_problem* problem,
    const mmx_gn_options* options,
    double* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    void* stream);

/*
 * mmx_solve with SolverT::setStoreHistory(true) (momentum/solver/solver.cpp:53-72,101-110): additionally
 *   parameter_history  float [B][max_iterations][P]  iterationHistory_["parameters"]: the parameters after
 *                      iteration i; rows from an element's iteration count on stay zero (setZero(), :70)
 * (error_history is iterationHistory_["error"], `iterations` iterationHistory_["iterations"]).  The "jtj"
 * history of GaussNewtonSolverT (gauss_newton_solver.cpp:265-278) is not stored -- n^2 floats per element and
 * iteration --; it is J^T J at the parameters BEFORE iteration i, which mmx_eval_normal_equations returns for
 * row i-1 of parameter_history (theta_init for i = 0); the host mirror rebuilds it that way on request
 * (momentum_amd/capi.py Problem.jtj_history: lower triangle + regularization on the diagonal, like :249 leaves
 * hessianApprox_).
 */
int32_t mmx_solve_with_history(
    mmx_problem* problem,
    const mmx_gn_options* options,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    float* parameter_history,
    void* stream);

/*
 * mmx_solve_with_history + the LM schedule's decisions (MMX_STEP_LM_SCHEDULE; MMX_ERR_INVALID_ARGUMENT for the other step
 * rules when step_history is not null):
 *   step_history  double [B][max_iterations][2]  (lambda iteration i factored with, its gain ratio rho = actual / predicted
 *                 decrease -- the quantity TrustRegionQRT compares with 0.25 / 0.75 / nu,
 *                 momentum/character_solver/trust_region_qr.cpp:244-268; -1 when no step could be computed); rows from an
 *                 element's iteration count on stay zero.
 * A step is accepted iff rho > 0; lambda is multiplied by lm_up when !(rho >= 0.25), by lm_down when rho > 0.75.  With this
 * output a caller (and tests/test_gpu_baseline_parity.py) can tell an element whose answer differs from another precision's
 * because a gain ratio sat on a threshold from one that differs for any other reason.  Every route; parameter_history may be
 * null.
 */
int32_t mmx_solve_with_step_history(
    mmx_problem* problem,
    const mmx_gn_options* options,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    float* parameter_history,
    double* step_history,
    void* stream);

/*
 * Warm-started frame sequences in ONE launch: the serial per-frame loop of trackPosesForFrames
 * (marker_tracking/marker_tracker.cpp:905-913: every frame's solve starts from the previous frame's result) for S
 * independent sequences of F = num_frames frames.  Added without an ABI bump (no struct grows): a library that predates
 * the function lacks the symbol -- that is the feature probe.
 *   layout      the problem's batch is B = F x S instances, FRAME-MAJOR: instance f S + s is frame f of sequence s.  Every
 *               per-instance array keeps its meaning and its indexing by instance: the constraint payload,
 *               function_weights, per-instance rigs, all outputs, both histories.
 *   theta_dev   [F][S][P] (DEVICE).  In: the rows of frame 0 hold each sequence's initial parameters; the rows of later
 *               frames are NOT read.  Out: row f S + s holds frame f's result.
 *   meaning     frame f of sequence s is solved exactly -- bit for bit, on theta and on every output -- as mmx_solve on
 *               MMX_ROUTE_WAVE solves instance f S + s, started from the result row of frame f - 1 (f = 0: from the
 *               caller's row).  Nothing couples the frames except where the initial parameters come from.
 *   non-finite  a frame whose parameters end non-finite gets MMX_SOLVE_NONFINITE and its result row holds its own initial
 *               parameters (the driver's revert, tensor_ik.cpp:168-173); the next frame starts from that row.
 *   disabled parameters carry frame 0's values through every row.
 *   outputs     as mmx_solve_with_history (NULL to skip), [B] / [B][max_iterations] / [B][max_iterations][P].
 * One wavefront owns a sequence for all its frames (theta stays in its LDS; no launch, no host work and no wait for the
 * slowest sequence between frames), so the scope is MMX_ROUTE_WAVE's, see mmx_tuning.  Refusals, all before theta or any
 * output is touched:
 *   MMX_ERR_INVALID_ARGUMENT  num_frames < 1, or B is no multiple of num_frames
 *   MMX_ERR_UNSUPPORTED       a problem or options outside MMX_ROUTE_WAVE's scope (the route's own message); a
 *                             precision other than MMX_PRECISION_F32; a route pinned to anything but MMX_ROUTE_AUTO or
 *                             MMX_ROUTE_WAVE
 * mmx_problem_last_route answers MMX_ROUTE_WAVE afterwards; the routing of the other solve entry points is unchanged
 * (MMX_ROUTE_AUTO still never picks the wave route there).  Kernels only are enqueued (no memset node, no stream wait):
 * after one warm-up call the call can be captured into a HIP graph like the other solves.  The _host form copies in,
 * runs, copies out and synchronises like the other host wrappers.
 * Problems outside the wave route's scope (the one-launch and wide routes) are out of scope of this entry point for now:
 * the layout is chosen so that a host-driven form for them can keep it.
 */
int32_t mmx_solve_frames(
    mmx_problem* problem,
    const mmx_gn_options* options,
    int32_t num_frames,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    float* parameter_history,
    void* stream);
int32_t mmx_solve_frames_host(
    mmx_problem* problem,
    const mmx_gn_options* options,
    int32_t num_frames,
    float* theta_host,
    double* final_error_host,
    int32_t* iterations_host,
    int32_t* status_host);

/*
 * The error and the gradient of every instance WITHOUT a Jacobian: SkeletonSolverFunctionT::getGradient
 * (error_function_helpers.cpp:220) and getError in O(joints + constraints) per instance, through the skeleton tree (the
 * adjoint pass the wide route refines with), where mmx_eval_jacobian writes M x P floats per instance first.  Added without
 * an ABI bump (no struct grows): a library that predates the functions lacks the symbols -- that is the feature probe.
 *   meaning     with J and r as mmx_eval_jacobian returns them for the handle's current state (constraints, enabled mask,
 *               per-instance rig, losses, per-element function weights):
 *                 grad_dev [B][P]  grad[b][p] = 2 sum_i J[b][i][p] r[b][i].  All P entries of every row are written; the
 *                                  entries of disabled parameters and of structurally zero columns are exact zeros.
 *                                  (Also where J itself has an entry in a disabled column: a row of MMX_LIMIT_MINMAX_JOINT /
 *                                  MMX_LIMIT_LINEAR_JOINT carries every column of its transform row, enabled or not, like
 *                                  the reference's; a solve drops those columns, and so does the gradient.)
 *                 err_dev  [B]     the error mmx_eval_jacobian reports (under a robust loss the loss value, not |r|^2).
 *               The forward kinematics is the solve kernels' (pointer-jumping rounds in double), so err is the error a
 *               solve reports at theta; mmx_eval_jacobian keeps single-precision rounds, the two agree to rounding.
 *   forms       grad_dev == NULL: the error only (no moments, no tree sums); err_dev == NULL: the gradient only.  An
 *               output has the same bits whichever form produced it.  Both NULL: MMX_ERR_INVALID_ARGUMENT.
 *   scope       position and orientation blocks with every GeneralizedLoss the solves take; constraint, block and
 *               per-element function weights (columns 0-3); the parameter-space rows (every MMX_LIMIT_* type but the
 *               ellipsoid, the model-parameter prior); the enabled mask; per-instance offsets and pre-rotations.
 *   refusals    MMX_ERR_UNSUPPORTED with a message that names the condition, before any output is touched, the first
 *               that applies in this order: further joint-constraint blocks; ellipsoid limits; per-instance constraint
 *               parents; no position / orientation constraint or no solved parameter; tables beyond the kernel's LDS
 *               budget (160 KB).  There is no fallback through the Jacobian: those problems stay with mmx_eval_jacobian.
 *   determinism a row of the result depends on that instance's inputs only -- not on the batch size, the instance's
 *               position in the batch, or the run (no floating-point atomics; every entry is summed by one thread in a
 *               fixed order).
 * One kernel is enqueued on `stream` and the call returns (no memset node, no stream wait, no host read): after one
 * warm-up call it can be captured into a HIP graph like the solves.  The _host form copies in, runs, copies out and
 * synchronises like the other host wrappers.
 */
int32_t mmx_eval_gradient(mmx_problem* problem, const float* theta_dev, float* grad_dev, double* err_dev, void* stream);
int32_t mmx_eval_gradient_host(mmx_problem* problem, const float* theta_host, float* grad_host, double* err_host);

/*
 * The backward pass of mmx_eval_skeleton_state: the vector-Jacobian product of the skeleton state with a caller-supplied
 * cotangent, in O(joints + entries of the parameter transform) per instance through the skeleton tree (the adjoint pass of
 * mmx_eval_gradient with JOINTS as the units).  No state Jacobian (8 J x P) is formed.  The counterpart of _backward_kernel
 * in pymomentum/backend/triton_fk.py.  Added without an ABI bump (no struct grows): a library that predates the functions
 * lacks the symbols -- that is the feature probe.
 *   meaning     with state [B][J][8] = (tx,ty,tz, qx,qy,qz,qw, s) as mmx_eval_skeleton_state returns it for this handle at
 *               theta_dev, and L any scalar function of it:
 *                 state_grad_dev [B][J][8]  dL/dstate, in the layout of the state
 *                 theta_grad_dev [B][P]     dL/dtheta[b][p] = sum_{j,c} state_grad[b][j][c] dstate[b][j][c]/dtheta[b][p]
 *               The kernel recomputes the forward kinematics (the solve kernels': pointer-jumping rounds in double), so
 *               nothing has to be kept from a forward call.  It renormalises every local quaternion in double before the
 *               rounds: the exact composition of single-precision rotations lets the world quaternion's norm drift by up
 *               to 1e-6 down a long chain, which the state tolerates and a derivative of it does not; the state the
 *               derivative is taken at differs from the returned one by that drift.  Per-instance offsets and pre-rotations
 *               (mmx_problem_set_instance_rig) are read; the derivative is with respect to theta only.
 *   written     all P entries of every row.  A parameter without an entry in the parameter transform gets an exact zero.
 *               The enabled mask is NOT read (the forward does not read it either: a disabled parameter gets its true
 *               derivative), and joint pruning does not apply (every joint's state is an output).  Constraints are not read.
 *   quaternion  the cotangent is applied to the quaternion as the forward returns it: the same sign, and no
 *               renormalisation term of its own.  The state's quaternions are products of unit rotations, so the component
 *               of state_grad's quaternion part along q itself contributes nothing.
 *   refusals    before any output is touched: MMX_ERR_INVALID_ARGUMENT for a null pointer; MMX_ERR_UNSUPPORTED, with a
 *               message that names the condition, for a rig whose tables exceed the kernel's LDS budget (160 KB: beyond
 *               about 700 joints).  Every rig the one-launch solve takes is inside.
 *   determinism a row of the result depends on that instance's inputs only -- not on the batch size, the instance's
 *               position in the batch, or the run (no floating-point atomics; every entry is summed by one thread in a
 *               fixed order).
 * One kernel is enqueued on `stream` and the call returns (no memset node, no stream wait, no host read).  The rig-level
 * tables are built and uploaded by the first call on a rig: that call is the warm-up, after it the call can be captured into
 * a HIP graph like the other entry points.  The _host form copies in, runs, copies out and synchronises like the other host
 * wrappers.
 */
int32_t mmx_eval_skeleton_state_backward(
    mmx_problem* problem,
    const float* theta_dev,
    const float* state_grad_dev,
    float* theta_grad_dev,
    void* stream);
int32_t mmx_eval_skeleton_state_backward_host(
    mmx_problem* problem,
    const float* theta_host,
    const float* state_grad_host,
    float* theta_grad_host);

/*
 * Linear-blend skinning: skeleton state -> posed mesh vertices, and its backward pass.  The counterpart of _forward_kernel /
 * _backward_kernel in pymomentum/backend/triton_skinning.py (Character.skin_points) and of momentum's applySSD.  Added
 * without an ABI bump (no struct grows): a library that predates the functions lacks the symbols -- that is the feature probe.
 *
 * The skin (mmx_skin_desc) is static per character and shared by the batch; it mirrors momentum's SkinWeights and
 * Character::inverseBindPose.  joint / weight [V][K] with K <= MMX_MAX_SKIN_INFLUENCES; padding slots carry weight 0 and any
 * VALID joint index; weights are used as given (no renormalisation).  inverse_bind [J][12] is a 3 x 4 row-major affine
 * [A_j | a_j] per joint (the convention of mmx_joint_constraint_block::projection and mmx_ellipsoid_limit), NULL = identity.
 *   meaning     with (t_j, q_j, s_j) the row [b][j] of state [B][J][8] = (tx,ty,tz, qx,qy,qz,qw, s), r_v the rest position of
 *               vertex v (the skin's, or rest_dev [b][v] when that is not NULL: blend-shaped or identity-dependent meshes,
 *               the rest_vertices argument of skin_points) and p_vk = A_j r_v + a_j for j = joint[v][k]:
 *                 out [B][V][3]         out[b][v] = sum_k weight[v][k] ( t_j + s_j qrot(q_j, p_vk) )
 *                 state_grad [B][J][8]  dL/dstate for out_grad = dL/dout [B][V][3], in the layout of the state
 *                 rest_grad [B][V][3]   dL/dr[b][v] = sum_k weight[v][k] A_j^T ( s_j R(q_j)^T out_grad[b][v] ); optional
 *               qrot(q, p) = p + 2 w (u x p) + 2 u x (u x p) with q = (u, w).  The state may come from
 *               mmx_eval_skeleton_state or from anywhere else: the entry points take the state, not theta or a problem.
 *   quaternion  used exactly as the state holds it, not renormalised; state_grad is the exact derivative of the polynomial
 *               above, with no renormalisation term (what mmx_eval_skeleton_state_backward expects of its cotangent).
 *               Per joint everything follows from twelve sums over the joint's influences, F = sum w g and N = sum w g p^T:
 *               g_t = F, g_s = <R(q), N>, g_q = s d<R(q), N>/dq.
 *   written     every entry of out / state_grad / rest_grad.  A zero-weight slot contributes nothing, even when its joint's
 *               state is not finite; a joint without a non-zero-weight influence gets eight exact zeros in state_grad.
 *   refusals    before any output is touched: MMX_ERR_INVALID_ARGUMENT for a null required pointer, batch < 1, V < 1, K
 *               outside 1 .. 8, a joint index outside [0, J) in any slot (zero-weight ones included), a non-finite weight,
 *               inverse-bind entry or rest position at create; MMX_ERR_UNSUPPORTED at create, with a message that names the
 *               condition, for a rig whose posed affines (48 bytes per joint) exceed the kernels' LDS budget (160 KB:
 *               beyond 3412 joints).
 *   determinism a row of a result depends on that instance's inputs only -- not on the batch size, the instance's position
 *               in the batch, or the run.  The backward pass is a vertex-to-joint reduction without atomics: each joint's
 *               sums are taken by one wavefront over the joint's entries of the joint-sorted influence list
 *               (mmx_host_skin_tables) in a fixed order, lane = entry mod 64 and then a fixed cross-lane tree.
 * Streams and graphs: mmx_skin_points enqueues one kernel on `stream`, mmx_skin_points_backward one (two with rest_grad_dev)
 * and returns: no memset node, no stream wait, no host read, no device scratch; the tables are uploaded by mmx_skin_create.
 * The first call of a process raises a kernel attribute where a rig needs more than 64 KB of LDS: that call is the warm-up,
 * after it the calls can be captured into a HIP graph like the other entry points.  The _host forms take host arrays
 * (rest_host NULL or [B][V][3], rest_grad_host NULL to skip), copy in, run, copy out and synchronise like the other host
 * wrappers.  The handle keeps a reference to its rig, which must outlive it.
 *
 * mmx_host_skin_tables is the bookkeeping of the backward pass as a pure host function (no device): the joint-sorted
 * influence list, every (vertex, slot) pair with a non-zero weight sorted by (joint, vertex, slot), joint_start [J + 1] its
 * index.  entry_vertex / entry_slot hold up to V * K entries; any output may be NULL.  Only joint, weight and the two sizes
 * of the descriptor are read.  The backward kernel reads this list and nothing else to decide its summation order.
 *
 * PROVENANCE: this restates momentum's applySSD (SkinWeights, Character::inverseBindPose), pymomentum's
 * Character.skin_points and pymomentum/backend/triton_skinning.py from memory of the reference, without a checkout at hand, so
 * it carries no file:line citations yet.  To confirm against the reference: kMaxSkinJoints = 8; that weights are not
 * renormalised at skinning time; the transform order T_world * T_invbind.
 */
#define MMX_MAX_SKIN_INFLUENCES 8
typedef struct mmx_skin_desc {
  int32_t num_vertices;         /* V >= 1 */
  int32_t max_influences;       /* K, 1..MMX_MAX_SKIN_INFLUENCES (8) */
  const int32_t* joint;         /* [V][K] HOST */
  const float* weight;          /* [V][K] HOST */
  const float* inverse_bind;    /* [J][12] HOST, NULL = identity */
  const float* rest_positions;  /* [V][3] HOST */
} mmx_skin_desc;
typedef struct mmx_skin mmx_skin;

int32_t mmx_skin_create(mmx_rig* rig, const mmx_skin_desc* desc, mmx_skin** out);
void mmx_skin_destroy(mmx_skin* skin);
int32_t mmx_skin_num_vertices(const mmx_skin* skin);
int32_t mmx_skin_points(
    mmx_skin* skin,
    int32_t batch,
    const float* state_dev,
    const float* rest_dev /* NULL or [B][V][3] */,
    float* out_dev,
    void* stream);
int32_t mmx_skin_points_backward(
    mmx_skin* skin,
    int32_t batch,
    const float* state_dev,
    const float* rest_dev,
    const float* out_grad_dev,
    float* state_grad_dev,
    float* rest_grad_dev /* NULL to skip */,
    void* stream);
int32_t mmx_skin_points_host(mmx_skin* skin, int32_t batch, const float* state_host, const float* rest_host, float* out_host);
int32_t mmx_skin_points_backward_host(
    mmx_skin* skin,
    int32_t batch,
    const float* state_host,
    const float* rest_host,
    const float* out_grad_host,
    float* state_grad_host,
    float* rest_grad_host);
int32_t mmx_host_skin_tables(
    int32_t num_joints,
    const mmx_skin_desc* desc,
    int32_t* joint_start /* [J+1] */,
    int32_t* entry_vertex,
    int32_t* entry_slot,
    int32_t* num_entries);

/*
 * Gauss-Newton terms of vertex constraints on a skinned mesh: H = J^T J, g = J^T (sigma f) and the error of a batch of
 * constraints on a mmx_skin, over the problem's enabled parameters -- the counterpart of mmx_eval_normal_equations for the
 * skin, in its layout, so that the two sets of terms add and a caller takes the step theta -= (H + lambda I)^-1 g with a
 * batched Cholesky (the joint-constraint terms, limits and prior from mmx_eval_normal_equations added or not).  Nothing is
 * solved here and mmx_solve does not read these terms.  Added without an ABI bump (no struct grows): a library that predates
 * the functions lacks the symbols -- that is the feature probe.
 *   meaning     with out [B][V][3] exactly what mmx_skin_points gives (rest_dev of the descriptor: the per-instance rest, as
 *               there) on the state of mmx_eval_skeleton_state at theta, constraint c of instance b has the point
 *                 x_c = sum_{i < S} barycentric[b][c][i] out[b][vertex[b][c][i]]         S = corners: 1 or 3
 *               (S = 1: a mesh vertex, barycentric not read, weight 1; S = 3: a triangle's corners with barycentric weights,
 *               what mmx_closest_points_on_mesh returns) and the rows
 *                 MMX_VC_POSITION  f = x_c - target_c                three rows
 *                 MMX_VC_PLANE     f = normal_c . (x_c - target_c)   one row; normal_c used as given, not normalised
 *               scaled by sigma_c = sqrt(function_weight weight[b][c]); error = sum_c function_weight weight[b][c] |f|^2 --
 *               the weighting of the joint-constraint blocks, with no further constant.
 *   J           the exact derivative of the rows with respect to theta of the composed forward as this library defines it:
 *               the local quaternions renormalised in double (as in mmx_eval_skeleton_state_backward), the skin's quaternion
 *               used as the state holds it.  Row r of J is what mmx_eval_skeleton_state_backward(mmx_skin_points_backward(.))
 *               returns for the cotangent of row r.
 *   outputs     for the n enabled parameters, ascending -- the order and compaction of mmx_eval_normal_equations:
 *                 jtj_dev [B][n][n] float  full and exactly symmetric      jtr_dev [B][n] float  same sign: a step is theta -= delta
 *                 err_dev [B] double
 *               Any may be NULL (not all three); an output has the same bits whichever others were requested.  Every entry is
 *               written: an enabled parameter that moves no constrained vertex gets exact zeros.
 *   skipped     a constraint contributes exact zeros when weight[b][c] is not > 0 (zero, negative, NaN) or any of its vertex
 *               indices is negative (face_index = -1 of the closest-point kernels) or >= V; such an index is never
 *               dereferenced and nothing else of the constraint is read.  Non-finite targets or normals behind a positive
 *               weight are ordinary inputs: that instance's results are non-finite, no other's.
 *   arrays      vertex [B][C][S] int32, NULL only with S = 1 and C = V (constraint c is vertex c); barycentric [B][C][S],
 *               NULL when S = 1; target [B][C][3]; normal [B][C][3], MMX_VC_PLANE only; weight [B][C], NULL = every weight
 *               1; rest [B][V][3] or NULL.  B is the problem's batch.
 *   refusals    before any output is touched, with a message naming the condition: MMX_ERR_INVALID_ARGUMENT for a skin on
 *               another rig, a null required pointer, all outputs null, count < 1, corners outside {1, 3}, an unknown type,
 *               MMX_VC_PLANE without normals, a non-finite or negative function_weight; MMX_ERR_UNSUPPORTED for more than
 *               MMX_SKIN_NE_MAX_SOLVED (128) enabled parameters -- the accumulators of the kernel's four waves -- or tables
 *               beyond the kernel's LDS budget (160 KB).
 *   determinism an instance's results depend on that instance's inputs only -- not on the batch size, its position in the
 *               batch, or the run (no floating-point atomics; fixed summation order: rows ascending within an entry).
 * One kernel is enqueued on `stream` and the call returns (no memset node, no stream wait, no host read, no device scratch);
 * after one warm-up call (a kernel attribute is raised where the tables need more than 64 KB of LDS) it can be captured into a
 * HIP graph.  The _host form takes host arrays in the descriptor and for theta and the outputs, copies in, runs, copies out
 * and synchronises like the other host wrappers.
 *
 * PROVENANCE: this restates momentum's vertex error function (VertexErrorFunctionT, the Position and Plane constraint types)
 * from memory of the reference, without a checkout at hand, so it carries no file:line citations yet.  To confirm against
 * the reference: any constant factor on the weight (kPositionWeight / kPlaneWeight), and whether the plane normal is
 * normalised on ingest.  The Normal and SymmetricNormal types, which rotate the normal with the mesh, are not built.
 */
#define MMX_VC_POSITION 0
#define MMX_VC_PLANE 1
#define MMX_SKIN_NE_MAX_SOLVED 128
typedef struct mmx_vertex_constraints {
  int32_t type;             /* MMX_VC_* */
  int32_t count;            /* C >= 1 constraints per instance */
  int32_t corners;          /* S: 1 or 3 */
  float function_weight;    /* finite, >= 0 */
  const int32_t* vertex;    /* [B][C][S] or NULL */
  const float* barycentric; /* [B][C][S] or NULL */
  const float* target;      /* [B][C][3] */
  const float* normal;      /* [B][C][3] or NULL */
  const float* weight;      /* [B][C] or NULL */
  const float* rest;        /* [B][V][3] or NULL */
} mmx_vertex_constraints;
int32_t mmx_skin_normal_equations(
    mmx_problem* problem,
    mmx_skin* skin,
    const mmx_vertex_constraints* constraints /* DEVICE arrays */,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    double* err_dev,
    void* stream);
int32_t mmx_skin_normal_equations_host(
    mmx_problem* problem,
    mmx_skin* skin,
    const mmx_vertex_constraints* constraints /* HOST arrays */,
    const float* theta_host,
    float* jtj_host,
    float* jtr_host,
    double* err_host);

/*
 * The same terms with every instance's 32-row tiles divided over `parts` workgroups: for the shape a mesh fit has -- one
 * scan or a short clip against a dense mesh -- where one workgroup per instance leaves the device idle.  Added without an ABI
 * bump: the new symbols are the feature probe.  mmx_skin_normal_equations itself, its results and its defaults do not change.
 *   meaning     everything mmx_skin_normal_equations documents (rows, sigma, J, skipped constraints, layout, sign) holds
 *               unchanged.  With rows = C (MMX_VC_PLANE) or 3 C (MMX_VC_POSITION), T = ceil(rows / 32) tiles and
 *               Pe = min(parts, T), part p owns the tiles [floor(p T / Pe), floor((p + 1) T / Pe)) -- no part is empty.  Tile
 *               composition is that of the unsplit kernel (it depends on C, S and the type only); a position constraint
 *               that straddles a part boundary is evaluated in both parts and writes the rows that fall in each.  Part p
 *               produces the float32 matrix-core accumulators of the lower block triangle over its tiles (tiles ascending,
 *               from zero), per column the double h0 + h1 of the unsplit kernel's g reduction over its tiles, and its 32
 *               row threads' double error sums added in row order.  A second kernel writes, for every entry,
 *                 H = float(sum_p double(acc_p))     g = float(sum_p g_p)     err = sum_p err_p
 *               each sum over p ascending, in double, rounded once; H is mirrored as in the unsplit kernel, so it is
 *               bitwise symmetric.  Every entry of every requested output is written; an output's bits do not depend on
 *               which others were requested.
 *   parts       1..MMX_SKIN_NE_MAX_PARTS, or 0 = the value mmx_skin_normal_equations_auto_parts reports.  An effective
 *               parts of 1 (parts = 1, or T = 1) IS mmx_skin_normal_equations: its bits, one kernel node, the workspace
 *               neither needed nor touched.  parts >= T gives the bits of parts = T.
 *   workspace   device memory of at least mmx_skin_normal_equations_workspace_bytes(B, n, parts) bytes (n = the enabled
 *               parameters; the size is taken for the parts asked for -- for parts = 0 the value it resolves to -- not for
 *               Pe), 16-byte aligned; may be NULL / 0 when the effective parts is 1.  It is written before it is read:
 *               its prior contents never reach a result, and it holds nothing a later call needs.
 *   refusals    before any output or the workspace is touched, with a message naming the condition: every refusal of
 *               mmx_skin_normal_equations, in its order, first; then MMX_ERR_INVALID_ARGUMENT for parts < 0 or
 *               parts > MMX_SKIN_NE_MAX_PARTS, for a null workspace or workspace_bytes below the size above when Pe > 1,
 *               and for a workspace that is not 16-byte aligned.  The _host form stages its arrays first and then
 *               refuses in the same order.
 *   determinism an instance's results depend on that instance's inputs and on Pe only -- not on the batch size, its
 *               position in the batch, or the run (no atomics, no inter-workgroup synchronisation; the parts are added in a
 *               fixed order).  Different Pe give results that differ in the last bits (the association of the sums).
 *               parts = 0 therefore depends on the batch size, through the plan only: a caller who wants identical bits
 *               across batch sizes pins `parts`.
 *   plan        mmx_skin_normal_equations_plan (pure host, no device touched):
 *                 parts = max(1, min(floor(compute_units workgroups_per_cu / batch), T, MMX_SKIN_NE_MAX_PARTS))
 *               -- the device's workgroup slots per instance, as far as the tiles reach.  Every part repeats the set-up
 *               (forward kinematics, posed affines, column sources), yet a part of a single tile was the fastest choice
 *               at every measured shape; only humanoid72 p128 was measured.  MMX_ERR_INVALID_ARGUMENT, nothing written, for batch < 1, count < 1, an unknown type,
 *               compute_units < 1 or workgroups_per_cu < 1.  mmx_skin_normal_equations_auto_parts feeds it the device's
 *               compute-unit count and workgroups_per_cu = 2 where two workgroups' LDS fit in 160 KB, else 1; it refuses what
 *               mmx_skin_normal_equations refuses of the problem, skin and descriptor's type, count and corners (the
 *               arrays are not read and may be NULL).
 * Two kernels are enqueued on `stream` (one when the effective parts is 1) and the call returns: no memset node, no stream
 * wait, no host read; after one warm-up call it can be captured into a HIP graph as a linear chain of two kernel nodes.
 * The _host form takes host arrays like mmx_skin_normal_equations_host and allocates and frees its own workspace.
 */
#define MMX_SKIN_NE_MAX_PARTS 512 /* 256 CUs x two workgroups per CU at one instance */
int32_t mmx_skin_normal_equations_split(
    mmx_problem* problem,
    mmx_skin* skin,
    const mmx_vertex_constraints* constraints /* DEVICE arrays */,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    double* err_dev,
    int32_t parts,
    void* workspace_dev,
    int64_t workspace_bytes,
    void* stream);
int32_t mmx_skin_normal_equations_split_host(
    mmx_problem* problem,
    mmx_skin* skin,
    const mmx_vertex_constraints* constraints /* HOST arrays */,
    const float* theta_host,
    float* jtj_host,
    float* jtr_host,
    double* err_host,
    int32_t parts);
/* pure host: bytes a call needs; 0 for parts <= 1; -1 for batch < 1, num_enabled outside 1..128 or parts outside 0..512 */
int64_t mmx_skin_normal_equations_workspace_bytes(int32_t batch, int32_t num_enabled, int32_t parts);
int32_t mmx_skin_normal_equations_plan(
    int32_t batch,
    int32_t type,
    int32_t count,
    int32_t compute_units,
    int32_t workgroups_per_cu,
    int32_t* parts_out);
int32_t mmx_skin_normal_equations_auto_parts(
    mmx_problem* problem,
    mmx_skin* skin,
    const mmx_vertex_constraints* constraints,
    int32_t* parts_out);
/* pure host: the tiles [*begin_out, *end_out) that part `part` of a call with `parts` parts over `tiles` tiles owns, and
 * *effective_parts_out = min(parts, tiles) (any output may be NULL); MMX_ERR_INVALID_ARGUMENT, nothing written, for tiles < 1,
 * parts outside 1..MMX_SKIN_NE_MAX_PARTS or part outside [0, min(parts, tiles)) */
int32_t mmx_skin_normal_equations_part_range(
    int32_t tiles,
    int32_t parts,
    int32_t part,
    int32_t* begin_out,
    int32_t* end_out,
    int32_t* effective_parts_out);

/*
 * Batched nearest-point queries: for every source point of every instance, the index of the nearest eligible target point
 * of the same instance (and, optionally, its squared distance and the point itself).  The counterpart of
 * pymomentum.geometry.find_closest_points and of its overload with normals, which run on the CPU; what an ICP loop does
 * with the posed vertices of mmx_skin_points in every iteration.  Stateless: no handle, the arrays are the call's only
 * state, on the current device.  Added without an ABI bump (no struct grows): a library that predates the functions lacks
 * the symbols -- that is the feature probe.
 *   distance    for source s and target t, dx = s.x - t.x, dy = s.y - t.y, dz = s.z - t.z taken FIRST, in float32, then
 *                 d2 = fma(dz, dz, fma(dy, dy, dx * dx))
 *               -- the same instruction sequence for every pair, whichever lane, wave, tile or remainder handles it, so
 *               two identical target points compute identical bits.  The expanded form |s|^2 + |t|^2 - 2 s.t is not
 *               used anywhere (in float32 it picks wrong neighbours as soon as the cloud sits away from the origin).
 *   eligible    a pair is eligible when d2 is finite, d2 <= max_dist * max_dist (the product taken in float32: +inf stays
 *               +inf) and, with normals, fma(ns.z, nt.z, fma(ns.y, nt.y, ns.x * nt.x)) >= min_normal_dot.  Normals are
 *               used as given, not renormalised.  Both normal arrays or neither.
 *   non-finite  every comparison is ordered, so a NaN anywhere in a pair (a coordinate, a normal) makes the pair
 *               ineligible; so does an infinite coordinate (d2 is then +inf or NaN).  These are ordinary inputs.
 *   result      the eligible target with the smallest computed d2; among targets with equal computed d2 the lowest index.
 *               index [B][N] is -1 where no target is eligible; dist2 (optional) is the winning computed d2, +inf where
 *               index is -1; points (optional) is a copy of the winning target's three floats, zeros where index is -1.
 *               Every entry of every non-NULL output is written.
 *   sharing     target_shared != 0: one target cloud [M][3] (and its normals [M][3]) serves every instance; the result is
 *               bit-identical to the same cloud replicated per instance.
 *   refusals    before any output is touched: MMX_ERR_INVALID_ARGUMENT for a null required pointer (source, target, index),
 *               batch, num_source or num_target below 1, max_dist negative or NaN, exactly one of the two normal arrays,
 *               min_normal_dot NaN when normals are given, a launch grid beyond 2^31 - 1 workgroups.
 *   determinism a row of a result depends on that instance's inputs only -- not on the batch size, the instance's position
 *               in the batch, or the run.  No atomics: a lane scans its targets in ascending order with a strict <, and
 *               where a tile's targets are divided over waves the partial results are combined in a fixed order by the
 *               lexicographic minimum of (d2, index).
 * Streams and graphs: mmx_closest_points enqueues ONE kernel on `stream` and returns: no memset node, no stream wait, no
 * host read, no device scratch, no kernel attribute to raise (the kernel needs 32 KB of LDS).  It can be captured into a HIP
 * graph from the first call on.  mmx_closest_points_host takes host arrays, copies in, runs, copies out and synchronises
 * like the other host wrappers.
 *
 * mmx_closest_points_plan is the launch decision as a pure host function (no device), the one the launcher itself calls:
 * how many sources a workgroup owns, how many targets a staged LDS tile holds, and over how many waves a tile's targets are
 * divided (1 would mean not divided; the kernel as built always divides a tile over its four waves, which all hold the
 * same sources).  MMX_ERR_INVALID_ARGUMENT for a size below 1 or a grid beyond 2^31 - 1; any output may be NULL.
 *
 * PROVENANCE: this restates pymomentum.geometry.find_closest_points (points_source, points_target, max_dist) ->
 * (closest_points, index, valid) and its overload with normals from memory of the reference, without a checkout at hand,
 * so it carries no file:line citations yet.  To confirm against the reference: the name and the default of the normal
 * threshold (remembered as max_normal_dot, default 0; here min_normal_dot, the dot product's lower bound), whether the
 * reference compares with >= or >, and whether its max_dist test is <= or <.
 */
int32_t mmx_closest_points(
    int32_t batch,
    int32_t num_source,
    int32_t num_target,
    const float* source_dev /* [B][N][3] */,
    const float* target_dev /* [B][M][3], or [M][3] when target_shared != 0 */,
    int32_t target_shared,
    const float* source_normals_dev /* NULL or [B][N][3] */,
    const float* target_normals_dev /* NULL or laid out like target_dev; both or neither */,
    float max_dist /* >= 0, +inf allowed */,
    float min_normal_dot /* read only with normals */,
    int32_t* index_dev /* [B][N], -1 = no eligible target */,
    float* dist2_dev /* NULL or [B][N], +inf where index is -1 */,
    float* points_dev /* NULL or [B][N][3], zeros where index is -1 */,
    void* stream);
int32_t mmx_closest_points_host(
    int32_t batch,
    int32_t num_source,
    int32_t num_target,
    const float* source_host,
    const float* target_host,
    int32_t target_shared,
    const float* source_normals_host,
    const float* target_normals_host,
    float max_dist,
    float min_normal_dot,
    int32_t* index_host,
    float* dist2_host,
    float* points_host);
int32_t mmx_closest_points_plan(
    int32_t batch,
    int32_t num_source,
    int32_t num_target,
    int32_t with_normals,
    int32_t* sources_per_workgroup,
    int32_t* target_tile,
    int32_t* target_ways);

/*
 * Vertex normals of a batch of posed triangle meshes, and their backward pass.  The counterpart of
 * pymomentum.geometry.compute_vertex_normals(vertex_positions, triangles) and of momentum's Mesh::updateNormals; what feeds
 * the normals_source / normals_target arguments of mmx_closest_points from the posed vertices of mmx_skin_points without
 * leaving the device.  Added without an ABI bump (no struct grows): a library that predates the functions lacks the symbols
 * -- that is the feature probe.
 *
 * A mesh handle (mmx_mesh) holds V >= 1 vertices and T >= 1 triangles tri [T][3] (int32 vertex indices); it is static and
 * shared by the batch.
 *   face vector for positions p [B][V][3] and triangle t = (a, b, c):   c_t = (p_b - p_a) x (p_c - p_a)
 *               in the triangle's own corner order and NOT normalised, so the normals are area-weighted.  It is computed by
 *               one instruction sequence: a triangle's face vector has the same bits at each of its three vertices.  The
 *               cross product rounds both products of a component and is never fused, so a triangle with a repeated
 *               vertex contributes three exact zeros in any corner order.
 *   vertex sum  m_v = sum of c_t over the incidence entries of v in ascending (triangle, corner) order (mmx_host_mesh_tables),
 *               added by one lane in that order.  A vertex at two corners of one triangle has two entries.
 *   normal      with s = |m_v|^2 taken in double:
 *                 s == 0 (an isolated vertex, or only degenerate faces)   n_v = three exact zeros     h_v = 0
 *                 s not finite                                            n_v = three NaNs            h_v = NaN
 *                 otherwise                                               n_v = m_v / sqrt(s)         h_v = (g_v - n_v (n_v . g_v)) / |m_v|
 *               Non-finite positions are ordinary inputs, not an error: a NaN position gives NaN normals on that vertex's
 *               closed 1-ring and nowhere else.  A NaN normal makes every pair it is part of ineligible in
 *               mmx_closest_points (its comparisons are ordered), which is the wanted composition; a ZERO normal has dot
 *               product 0 with everything and is therefore ELIGIBLE at the default min_normal_dot = 0.
 *   backward    for g = dL/dn [B][V][3] and h_v as above (from the stored sums):  H_t = (h_a + h_b) + h_c, the same bits
 *               wherever it is used, and
 *                 position_grad[b][x] = sum over the entries (t, corner of x) of (p_next - p_prev) x H_t
 *               with next / prev cyclic in (a, b, c), in the same ascending entry order as the forward.  This is the exact
 *               derivative of the forward (no term is dropped).
 *   written     every entry of normals, sums (when not NULL) and position_grad.
 *   refusals    before any output is touched and before the first HIP call, with a message that starts with the function's
 *               name: MMX_ERR_INVALID_ARGUMENT for a null required pointer, V, T or batch below 1, an index outside [0, V),
 *               3 T or B V 3 beyond 2^31 - 1, a grid beyond 2^31 - 1 workgroups; at create also for an incidence list
 *               whose device layout (each group of 64 vertices padded to the group's highest valence) exceeds 2^31 - 1
 *               records.
 *   determinism a row of a result depends on that instance's positions and cotangent only -- not on the batch size, the
 *               instance's position in the batch, or the run.  Both kernels are gathers, one lane per vertex: no atomics.
 *   cost        a face vector is recomputed at each of its three vertices (the alternative needs scratch or atomics).  A
 *               vertex of very high valence (the hub of a fan) is walked by ONE lane: correct, but slow.
 * Streams and graphs: mmx_vertex_normals and mmx_vertex_normals_backward each enqueue exactly ONE kernel on `stream` and
 * return: no memset node, no stream wait, no host read, no device scratch (which is why the backward takes sums_dev, the
 * m_v the forward wrote, instead of recomputing a 2-ring); the tables are uploaded by mmx_mesh_create.  The calls can be
 * captured into a HIP graph from the first call on.
 *
 * The _host forms take the mesh itself (sizes, host triangles, device ordinal) and host arrays instead of a handle: they
 * refuse like mmx_mesh_create and the device forms together, still without a device, then create a handle, copy in, run,
 * copy out, synchronise and destroy the handle -- the convenience form; a loop keeps a handle and calls the device forms.
 *
 * mmx_host_mesh_tables is the bookkeeping as a pure host function (no device): the vertex-sorted incidence list, every
 * (triangle, corner) pair sorted by (vertex, triangle, corner), vertex_start [V + 1] its index; entry_triangle / entry_corner
 * hold 3 T entries; max_valence is the longest list.  Any output may be NULL.  The kernels read this list (transposed per 64
 * vertices) and nothing else to decide their summation order.
 *
 * PROVENANCE: this restates pymomentum.geometry.compute_vertex_normals(vertex_positions, triangles) and momentum's
 * Mesh::updateNormals from memory of the reference, without a checkout at hand, so it carries no file:line citations yet.
 * To confirm against the reference: that face vectors are area-weighted and not normalised per face; what the reference does
 * with a NaN face (it may skip it; here it propagates); what it does with a zero sum (here: a zero normal).
 */
typedef struct mmx_mesh mmx_mesh;
int32_t mmx_mesh_create(int32_t num_vertices, int32_t num_triangles, const int32_t* triangles /* [T][3] HOST */, int32_t device, mmx_mesh** out);
void mmx_mesh_destroy(mmx_mesh* mesh);
int32_t mmx_mesh_num_vertices(const mmx_mesh* mesh);
int32_t mmx_mesh_num_triangles(const mmx_mesh* mesh);
int32_t mmx_vertex_normals(
    mmx_mesh* mesh,
    int32_t batch,
    const float* positions_dev /* [B][V][3] */,
    float* normals_dev /* [B][V][3] */,
    float* sums_dev /* NULL or [B][V][3]: m_v, what the backward reads */,
    void* stream);
int32_t mmx_vertex_normals_backward(
    mmx_mesh* mesh,
    int32_t batch,
    const float* positions_dev,
    const float* sums_dev /* required */,
    const float* normal_grad_dev,
    float* position_grad_dev,
    void* stream);
int32_t mmx_vertex_normals_host(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t device,
    int32_t batch,
    const float* positions_host,
    float* normals_host,
    float* sums_host /* NULL to skip */);
int32_t mmx_vertex_normals_backward_host(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t device,
    int32_t batch,
    const float* positions_host,
    const float* sums_host,
    const float* normal_grad_host,
    float* position_grad_host);
int32_t mmx_host_mesh_tables(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t* vertex_start /* [V+1] */,
    int32_t* entry_triangle,
    int32_t* entry_corner /* up to 3T each */,
    int32_t* num_entries,
    int32_t* max_valence);

/*
 * Closest points ON a posed triangle mesh (point-to-surface): for every source point of every instance, the nearest point
 * of the nearest eligible triangle of the same instance's mesh, with its face index and barycentric coordinates.  The
 * counterpart of pymomentum.geometry.find_closest_points_on_mesh, which runs on the CPU; the last stage of
 * skeleton_state -> skin_points -> closest points in a registration loop, where the residual slides along the surface and a
 * gradient reaches all three vertices of the face.  Added without an ABI bump (no struct grows): a library that predates
 * the functions lacks the symbols -- that is the feature probe.  All arrays are float32 (indices int32) on the mesh's device.
 *
 * For source p and triangle f = (a, b, c) of the handle's list, vertices [B][V][3] (or one shared [V][3]):
 *   record      (per triangle, one function)  e1 = b - a, e2 = c - a, float32 differences; the face vector n = e1 x e2 as
 *               mmx_vertex_normals computes it (both products of a component rounded, never fused), here in float32;
 *                 d11 = dot(e1, e1)  d12 = dot(e2, e1)  d22 = dot(e2, e2)     dot(u, w) = fma(u.z, w.z, fma(u.y, w.y, u.x * w.x))
 *                 i11 = 1 / d11   i22 = 1 / d22   ibc = 1 / ((d11 - d12) + (d22 - d12))
 *               (correctly rounded divisions).  The triangle is INELIGIBLE FOR EVERY SOURCE when n is three exact zeros
 *               (a repeated vertex index gives that) or when any of the fifteen record values is not finite.
 *   pair        (per source and triangle, one function)  v = p - a taken FIRST, in float32; then the region form of
 *               Ericson, Real-Time Collision Detection 5.1.5, branch-free (selects applied in reverse order of priority):
 *                 d1 = dot(e1, v)  d2 = dot(e2, v)  d3 = d1 - d11  d4 = d2 - d12  d5 = d1 - d12  d6 = d2 - d22
 *                 vc = fma(d1, d4, -(d3 * d2))   vb = fma(d5, d2, -(d1 * d6))   va = fma(d3, d6, -(d5 * d4))
 *                 (s, t) = (vb * den, vc * den), den = rcp((va + vb) + vc)                   the interior (rcp: the hardware
 *                                                                                            reciprocal, within 1 ulp)
 *                        = (1 - w, w), w = (d4 - d3) * ibc   if va <= 0, d4 - d3 >= 0, d5 - d6 >= 0    edge bc
 *                        = (0, d2 * i22)                     if vb <= 0, d2 >= 0, d6 <= 0              edge ac
 *                        = (0, 1)                            if d6 >= 0, d5 <= d6                      vertex c
 *                        = (d1 * i11, 0)                     if vc <= 0, d1 >= 0, d3 <= 0              edge ab
 *                        = (1, 0)                            if d3 >= 0, d4 <= d3                      vertex b
 *                        = (0, 0)                            if d1 <= 0, d2 <= 0                       vertex a
 *                 (the LAST line that applies wins), then with q(x) = 1 - (1 - x), which rounds x in [0, 1] to a multiple of
 *                 2^-24:  s = q(min(max(s, 0), 1)),  t = q(min(max(t, 0), 1 - s)).  That moves the point by less than a unit in
 *                 the last place of an edge and makes 1 - s and (1 - s) - t exact: the weights sum to 1 without rounding.  Then
 *                 r = fma(-t, e2, fma(-s, e1, v))  per component,   dist2 = fma(r.z, r.z, fma(r.y, r.y, r.x * r.x)).
 *               dist2 is |r|^2 of the RESIDUAL VECTOR; the expanded quadratic |v|^2 - 2 s (e1.v) - ... is not used anywhere
 *               (in float32 it is wrong by thousands of units in the last place of the pair's scale near the surface).
 *               Every pair goes through this instruction sequence and no other, whichever lane, wave, tile or remainder
 *               handles it (no contraction is left to the compiler), so two identical triangles compute identical bits.
 *   eligible    dist2 is finite and dist2 <= max_dist * max_dist (the product taken in float32: +inf stays +inf).  Every
 *               comparison is ordered, so a NaN or an infinity anywhere in a pair makes the pair ineligible.  Non-finite
 *               sources and vertices are ordinary inputs, not errors.
 *   result      the eligible triangle with the smallest computed dist2; among equal dist2 the lowest face index.
 *               face_index [B][N] is -1 where nothing is eligible; barycentric [B][N][3] = (w_a, w_b, w_c) with w_b = s,
 *               w_c = t, w_a = (1 - s) - t (exact; each >= 0 by the clamps above); points [B][N][3] = fma(t, e2, fma(s, e1, a))
 *               per component; dist2 [B][N] the winning computed dist2.  Where face_index is -1 the barycentrics and the
 *               points are zeros and dist2 is +inf.  Every entry of every non-NULL output is written.
 *   sharing     vertices_shared != 0: one [V][3] array serves every instance; the result is bit-identical to the same
 *               vertices replicated per instance.
 *   refusals    before any output is touched and before the first HIP call, with a message that starts with the function's
 *               name: MMX_ERR_INVALID_ARGUMENT for a null required pointer (mesh, source, vertices, face_index), batch or
 *               num_source below 1, max_dist negative or NaN, a launch grid beyond 2^31 - 1 workgroups; the _host form also
 *               for what mmx_mesh_create refuses.
 *   determinism a row of a result depends on that instance's inputs only -- not on the batch size, the instance's position
 *               in the batch, or the run.  No atomics: a lane scans its faces in ascending order with a strict <, and the
 *               partial results of the waves that share a tile are combined by the lexicographic minimum of (dist2, face).
 * Streams and graphs: mmx_closest_points_on_mesh enqueues ONE kernel on `stream` and returns: no memset node, no stream wait,
 * no host read, no device scratch, no kernel attribute to raise (38 KB of LDS).  The triangle list is uploaded by
 * mmx_mesh_create.  The call can be captured into a HIP graph from the first call on.  The _host form takes the mesh itself
 * (sizes, host triangles, device ordinal) and host arrays like mmx_vertex_normals_host: it refuses without a device, then
 * creates a handle, copies in, runs, copies out, synchronises and destroys the handle.
 *
 * mmx_closest_points_on_mesh_plan is the launch decision as a pure host function (no device), the one the launcher itself
 * calls: how many sources a workgroup owns, how many triangles a staged LDS tile holds, and over how many waves a tile's
 * triangles are divided.  MMX_ERR_INVALID_ARGUMENT for a size below 1 or a grid beyond 2^31 - 1; any output may be NULL.
 *
 * PROVENANCE: this restates pymomentum.geometry.find_closest_points_on_mesh(points_source, vertices_target, faces_target) ->
 * (valid, closest_points, face_index, barycentric) from memory of the reference, without a checkout at hand, so it carries no
 * file:line citations yet.  To confirm against the reference: the order of the returned tuple; the order of the barycentric
 * weights (here the face's own corner order a, b, c); what the reference does with degenerate faces (here they are never
 * returned); and that it has no max_dist (here an extension; +inf reproduces a call without it).
 */
int32_t mmx_closest_points_on_mesh(
    mmx_mesh* mesh,
    int32_t batch,
    int32_t num_source,
    const float* source_dev /* [B][N][3] */,
    const float* vertices_dev /* [B][V][3], or [V][3] when vertices_shared != 0 */,
    int32_t vertices_shared,
    float max_dist /* >= 0, +inf allowed */,
    int32_t* face_index_dev /* [B][N], -1 = no eligible triangle */,
    float* barycentric_dev /* NULL or [B][N][3], zeros where face_index is -1 */,
    float* points_dev /* NULL or [B][N][3], zeros where face_index is -1 */,
    float* dist2_dev /* NULL or [B][N], +inf where face_index is -1 */,
    void* stream);
int32_t mmx_closest_points_on_mesh_host(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t device,
    int32_t batch,
    int32_t num_source,
    const float* source_host,
    const float* vertices_host,
    int32_t vertices_shared,
    float max_dist,
    int32_t* face_index_host,
    float* barycentric_host /* NULL to skip */,
    float* points_host /* NULL to skip */,
    float* dist2_host /* NULL to skip */);
int32_t mmx_closest_points_on_mesh_plan(
    int32_t batch,
    int32_t num_source,
    int32_t num_triangles,
    int32_t* sources_per_workgroup,
    int32_t* triangle_tile,
    int32_t* triangle_ways);

/*
 * Numerical diagnostics of the LAST single-precision solve on this handle (one-launch and wide routes;
 * MMX_ERR_UNSUPPORTED after a solve on the explicit-Jacobian route or before the first solve): diag_dev [B][4] floats
 *   [0] the precision estimate MMX_SOLVE_PRECISION_SUSPECT is decided on (relative to |theta|)
 *   [1] smallest Cholesky pivot ratio d_jj / (H_jj + lambda) met in any iteration (~ 1 / cond(J^T J + lambda I))
 *   [2] largest |last refinement correction| / |step| of any iteration
 *   [3] |theta| of the result
 * Elements that MMX_PRECISION_AUTO re-solved in double keep the single-precision run's figures.
 */
int32_t mmx_problem_solve_diagnostics(mmx_problem* problem, float* diag_dev, void* stream);

/*
 * Parity hook of the fused solve kernel: its normal equations at theta (first iteration), over
 * the kernel's SOLVE list = enabled parameters whose Jacobian column is not structurally zero
 * (the others get an exact zero step, like in the reference where H row/col and g vanish).
 * jtj_dev [B][n*n] (J^T J without lambda), jtr_dev [B][n]; solve_list_host [<= P] receives the
 * parameter index of each compacted column, *num_solved = n.  Pass null device pointers to query
 * n / the list only.  theta is not modified.
 */
int32_t mmx_debug_fused_normal_equations(
    mmx_problem* problem,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    int32_t* solve_list_host,
    int32_t* num_solved,
    void* stream);

/*
 * Parity hook of the wide route's first stage: H = J^T J (LOWER triangle of the n x n system written, the rest zero)
 * and g = J^T r from the tree moments (treeNormalEquationsKernel), in the layout of mmx_eval_normal_equations but with
 * the columns in the solvers' ELIMINATION order (the solve list mmx_debug_fused_normal_equations reports: the enabled
 * parameters, every subtree's ahead of those of the joints above it), so that the two can be compared entry by entry
 * after that permutation.  Problems without structurally zero columns, inside the tree kernels' scope;
 * MMX_ERR_UNSUPPORTED otherwise.
 */
int32_t mmx_debug_tree_normal_equations(mmx_problem* problem, const float* theta_dev, float* jtj_dev, float* jtr_dev, void* stream);

/* Host-buffer convenience wrappers (the reference's boundary hands over host
 * memory): copy in, run on the handle's stream, copy out, synchronise. */
int32_t mmx_solve_host(
    mmx_problem* problem,
    const mmx_gn_options* options,
    float* theta_host,
    double* final_error_host,
    int32_t* iterations_host,
    int32_t* status_host);
int32_t mmx_solve_f64_host(
    mmx_problem* problem,
    const mmx_gn_options* options,
    double* theta_host,
    double* final_error_host,
    int32_t* iterations_host,
    int32_t* status_host);
int32_t mmx_eval_jacobian_host(
    mmx_problem* problem,
    const float* theta_host,
    float* jac_host,
    float* res_host,
    double* err_host,
    int32_t layout);
/* mmx_eval_skeleton_state with host buffers: theta_host [B][P] -> state_host [B][J][8] (tx,ty,tz, qx,qy,qz,qw, s). */
int32_t mmx_eval_skeleton_state_host(mmx_problem* problem, const float* theta_host, float* state_host);

/*
 * Multi-GPU: instances are independent, so a batch shards into contiguous blocks, one problem handle per
 * GPU, with NO collective on the data path (the reference runs one independent task per element,
 * pymomentum/tensor_ik/tensor_ik.cpp:127-177).  The one exchange is the per-batch residual norms -- (sum of
 * final errors, sum of iterations, number of failed instances), three doubles -- all-reduced once per solve
 * with RCCL over xGMI.  The communicator below is that all-reduce and nothing else; RCCL is called directly
 * (librccl is looked up at run time, so a single-GPU process never loads it).
 *   multi-process (one rank per GPU):  rank 0 calls mmx_comm_unique_id and hands the 128 bytes to the other
 *     ranks (any side channel: a torch.distributed / MPI broadcast, a file); every rank calls mmx_comm_create.
 *   single process (one host thread per GPU):  mmx_comm_create_all fills one communicator per device; the
 *     threads then call mmx_comm_all_reduce_norms concurrently (the C++ shell's BatchedMultiGpuSolver).
 */
#define MMX_COMM_ID_BYTES 128 /* NCCL_UNIQUE_ID_BYTES */
typedef struct mmx_comm mmx_comm;
int32_t mmx_comm_unique_id(uint8_t id[MMX_COMM_ID_BYTES]);
int32_t mmx_comm_create(const uint8_t id[MMX_COMM_ID_BYTES], int32_t world_size, int32_t rank, int32_t device, mmx_comm** out);
int32_t mmx_comm_create_all(int32_t num_devices, const int32_t* devices, mmx_comm** out /* [num_devices] */);
int32_t mmx_comm_world_size(const mmx_comm* comm);
int32_t mmx_comm_rank(const mmx_comm* comm);
/* In-place sum over the ranks of norms_dev[3] (DEVICE doubles) on `stream`; asynchronous like any kernel. */
int32_t mmx_comm_all_reduce_norms(mmx_comm* comm, double* norms_dev, void* stream);
/* The same for three HOST doubles: staged through a device buffer and a stream the communicator owns;
 * returns when norms_host holds the sums.  (Callers without device code, e.g. the C++ shell's threads.) */
int32_t mmx_comm_all_reduce_norms_host(mmx_comm* comm, double norms_host[3]);
/* (sum final_error, sum iterations, #elements with MMX_SOLVE_FAILED(status)) of a solve's outputs -> norms_dev[3], on `stream`. */
int32_t mmx_residual_norms(int32_t batch, const double* final_error, const int32_t* iterations, const int32_t* status, double* norms_dev, void* stream);
void mmx_comm_destroy(mmx_comm* comm);

/*
 * Host-side integer bookkeeping, exposed so that it can be checked bit-exactly
 * without a GPU (north_star: "bit-exact on joint-index bookkeeping").
 * All outputs are HOST arrays owned by the caller.
 *   level[J]            depth of each joint (root = 0)
 *   tin[J], tout[J]     DFS pre-order interval: a is an ancestor-or-self of j
 *                       iff tin[a] <= tin[j] < tout[a]
 *   active_joint_params[7J]  ParameterTransformT::computeActiveJointParams(enabled)
 *   enabled_list[P], *num_enabled  GaussNewtonSolverT::updateEnabledParameters
 */
int32_t mmx_host_tables(
    const mmx_rig_desc* desc,
    const uint8_t* enabled,
    int32_t* level,
    int32_t* tin,
    int32_t* tout,
    uint8_t* active_joint_params,
    int32_t* enabled_list,
    int32_t* num_enabled);

/*
 * The solvers' column order and the tile structure of their factor (host-side integer bookkeeping, no GPU needed).
 * The reference factors a dense J (QR); the step it computes does not depend on a column order, so the solvers here
 * number the columns of (J^T J + lambda I) in an ELIMINATION order: the enabled parameters sorted by the post-order
 * position (children before their parent, smaller subtrees first) of the last joint each drives.  Two columns of J
 * overlap only when a joint of the one is an ancestor-or-self of a joint of the other, so in that order the Cholesky
 * factor has no fill outside that pattern, and the blocked solvers of the wide route skip its all-zero 16 x 16 tiles.
 *   mmx_host_elimination_order: order[P] receives the enabled parameters in that order, *num_enabled their count.
 *   mmx_host_tile_structure: symbolic factorisation on the tile grid for an n x n pattern (related[n*n], row-major,
 *     entry (row, col), row > col, non-zero = H(row, col) can be non-zero; n <= 512): row_mask[32] (bit J of word I:
 *     tile (I, J <= I) of the factor is structurally non-zero), col_mask[32] (bit I of word k: tile (I >= k, k) is),
 *     *products = tile products L(I,j) L(k,j)^T the masked factorisation performs.
 *   mmx_problem_tile_structure: the masks the problem's wide route runs with (all ones when it keeps the dense
 *     structure: further joint error functions / ellipsoid limits present, or outside the tree kernels' scope).
 */
int32_t mmx_host_elimination_order(const mmx_rig_desc* desc, const uint8_t* enabled, int32_t* order, int32_t* num_enabled);
int32_t mmx_host_tile_structure(int32_t n, const uint8_t* related, uint32_t* row_mask, uint32_t* col_mask, int64_t* products);
/*
 *   mmx_host_live_joints: the live-joint bookkeeping of mmx_tuning::joint_pruning for a list of n referenced joints --
 *     live[J] (1 = the joint or one of its descendants is referenced), compact_of[J] (its index among the live joints,
 *     ascending in joint index, -1 for a dead joint), *num_live.  With no referenced joint nothing is pruned: every joint
 *     is live and compact_of is the identity.  Outputs may be null.  Host-only bookkeeping (additive).
 */
int32_t mmx_host_live_joints(const mmx_rig_desc* desc, int32_t n, const int32_t* joints, uint8_t* live, int32_t* compact_of, int32_t* num_live);
int32_t mmx_problem_tile_structure(mmx_problem* problem, uint32_t* row_mask, uint32_t* col_mask, int32_t* num_blocks, int32_t* num_tiles, int64_t* products);
/*
 *   mmx_host_tile_level_schedule: the order the resident factor kernel takes the block columns of that structure in --
 *     steps of mutually independent columns (no tile in each other's rows: different subtrees of the elimination tree),
 *     each column on its own waves of the 4-wave workgroup.  steps[0] = number of steps S, then 4 words per step:
 *     k | first_wave << 8 | num_waves << 12 (num_waves = 15: the whole workgroup, a panel beyond 208 rows) or -1.
 *     steps must hold 1 + 4 * 32 words.  Host-only bookkeeping (additive in ABI 9).
 */
int32_t mmx_host_tile_level_schedule(int32_t n, const uint8_t* related, int32_t* steps);
/*
 *   mmx_host_f64_assembly_list: what mmx_solve_f64 builds once per problem for its resident form -- per chunk of
 *     units_per_chunk constraint vectors (num_pos points, then three per orientation constraint) the entries (column c of
 *     solve_list, unit) of J that have an applicable source, with those sources' indices in the kernel's packed table
 *     (prefix sums of the columns' source counts in solve_list order + position in the column).  groups: two words per
 *     entry, c | unit-in-chunk << 12 | count << 18 and (count == 1 ? the source index : offset into extra);
 *     chunk_start: [chunks + 1] first group of a chunk, then [chunks] the chunk's mask of 16-column blocks with an entry.
 *     In: *num_groups / *num_extra = capacities of groups (in entries) / extra; out: the sizes (arrays are filled when
 *     they fit; call with null arrays to query).  chunk_start must hold 2 * chunks + 1 words.  Host-only (additive in ABI 9).
 */
int32_t mmx_host_f64_assembly_list(
    const mmx_rig_desc* desc,
    const int32_t* solve_list,
    int32_t n,
    const int32_t* pos_parent,
    int32_t num_pos,
    const int32_t* ori_parent,
    int32_t num_ori,
    int32_t units_per_chunk,
    uint32_t* groups,
    int32_t* num_groups,
    int32_t* extra,
    int32_t* num_extra,
    int32_t* chunk_start,
    int32_t* num_chunks);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* MMX_H_ */
