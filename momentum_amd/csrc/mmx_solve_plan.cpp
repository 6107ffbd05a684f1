// mmx_solve_plan.cpp -- see mmx_solve_plan.hpp.  The order of the checks below is the interface: where several refusals
// apply the first one is reported, and tests/cpp/test_solve_plan.cpp holds every one of them in its place.
#include "mmx_solve_plan.hpp"

namespace mmx {
namespace {

SolvePlan refuse(int32_t code, const char* message) {
  SolvePlan p;
  p.code = code;
  p.message = message;
  return p;
}

SolvePlan oneStage(const SolveStage& s) {
  SolvePlan p;
  p.numStages = 1;
  p.stages[0] = s;
  return p;
}

SolveStage stageOf(SolveStageKind kind, SolveStageSelect select, int32_t route) {
  SolveStage s;
  s.kind = kind;
  s.select = select;
  s.route = route;
  return s;
}

// MMX_PRECISION_MIXED (and MMX_PRECISION_AUTO's second stage): does the mixed-precision instantiation of the one-launch solve
// take this problem with these options?  Position / orientation constraints and the parameter-space rows; not the further joint
// error functions / ellipsoid limits, not the trust region, the route not pinned away from the one-launch solve.
bool mixedUsable(const SolveFacts& f, const mmx_gn_options& o) {
  return (f.route == MMX_ROUTE_AUTO || f.route == MMX_ROUTE_FUSED) && o.step_rule != MMX_STEP_TRUST_REGION && f.GT == 0 && f.U > 0 && f.n > 0 &&
      f.fusedUsable && f.fusedMixedUsable;
}

// The double kernel's LDS budget (its resident form always fits)
const char* f64Refusal(const SolveFacts& f) {
  return !f.f64Resident && f.f64LdsBytes > kPlanLdsBudget ? "mmx_solve_f64: rig beyond the kernel's LDS budget" : nullptr;
}

// One single-precision pass: the options, then the route.
SolvePlan planSingle(const SolveFacts& f, const mmx_gn_options& o, bool mayAbort) {
  if (const char* why = optionsRefusal(o, true)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, why);
  }
  SolveStage s = stageOf(SolveStageKind::Single, SolveStageSelect::All, MMX_ROUTE_WAVE);
  s.mayAbort = mayAbort;
  const int32_t route = f.route;
  if (route == MMX_ROUTE_WAVE) { // one wavefront per instance: taken only when pinned
    if (const char* why = waveRefusal(f, o, false)) {
      return refuse(MMX_ERR_UNSUPPORTED, why);
    }
    return oneStage(s);
  }
  // Systems of 129-224 solved parameters fit the one-launch solve only with one workgroup per CU (ten and more 16-blocks):
  // when the tree kernels cover the problem the wide route is the faster one, its factor is tile-sparse
  // (scripts/route_crossover.py).  The trust region's re-solve loops live in the one-launch solve; the wide route drives them
  // from the host, several small kernels per trust step: it takes the rule only where the one-launch solve cannot (no
  // instantiation, further joint error functions / ellipsoid limits) or when pinned.
  const bool trust = o.step_rule == MMX_STEP_TRUST_REGION;
  const bool fusedTakesRule = f.fusedUsable && !(trust && f.GT > 0);
  const bool wideWanted = route == MMX_ROUTE_WIDE || (trust ? !fusedTakesRule : f.fusedBlocks >= 10);
  const bool treeAllowed = f.treeUsable && route != MMX_ROUTE_FUSED && route != MMX_ROUTE_EXPLICIT_JACOBIAN;
  const bool preferWide = wideWanted && treeAllowed;
  const bool takeFused = fusedTakesRule && !preferWide && route != MMX_ROUTE_EXPLICIT_JACOBIAN;
  if (route == MMX_ROUTE_FUSED && !takeFused) {
    return refuse(MMX_ERR_UNSUPPORTED, "MMX_ROUTE_FUSED: the problem does not fit the one-launch solve (more than 224 solved parameters, or its tables beyond the LDS budget)");
  }
  if (route == MMX_ROUTE_WIDE && !preferWide) {
    return refuse(MMX_ERR_UNSUPPORTED, "MMX_ROUTE_WIDE: the problem is outside the tree kernels' scope");
  }
  if (takeFused) {
    s.route = MMX_ROUTE_FUSED;
    return oneStage(s);
  }
  if (trust && !preferWide) {
    return refuse(MMX_ERR_UNSUPPORTED, "MMX_STEP_TRUST_REGION: available in the one-launch solve and on the wide route (tree kernels); this problem takes neither (MMX_ROUTE_EXPLICIT_JACOBIAN, or outside the tree kernels' scope)");
  }
  if (f.solveN > kPlanMaxSolved) {
    return refuse(MMX_ERR_UNSUPPORTED, "more than 2048 solved parameters (kMaxModelParams; 512 on the tree routes, the explicit-Jacobian route takes the rest)");
  }
  // The host-driven routes.  Inside the tree kernels' scope, chosen above or because the in-LDS Cholesky step does not fit:
  // normal equations from the tree moments, left-looking factor in HBM, refinement through the tree, no dense J.  Else the
  // explicit Jacobian: dense J, J^T J on the matrix cores, the refinement streams J.
  s.wide = f.choleskyStepLdsBytes > kPlanLdsBudget;
  s.treeRefine = preferWide || (s.wide && treeAllowed);
  s.route = s.treeRefine ? MMX_ROUTE_WIDE : MMX_ROUTE_EXPLICIT_JACOBIAN;
  // (the trust region's host-driven re-factorisations and the explicit-Jacobian route keep MMX_SOLVE_DAMPING_FLOORED as their cue)
  s.wideDiag = s.treeRefine && !trust && f.refineSteps > 0;
  s.schedule = trust || o.step_rule == MMX_STEP_LM_SCHEDULE;
  s.deferred = s.schedule || o.do_line_search != MMX_LINE_SEARCH_NONE;
  return oneStage(s);
}

} // namespace

const char* preHandleRefusal(const mmx_gn_options& o, bool stepHistory) {
  if (stepHistory && o.step_rule != MMX_STEP_LM_SCHEDULE) {
    return "mmx_solve_with_step_history: step_history is the LM schedule's (MMX_STEP_LM_SCHEDULE)";
  }
  if (o.precision != MMX_PRECISION_F32 && o.precision != MMX_PRECISION_F64 && o.precision != MMX_PRECISION_AUTO && o.precision != MMX_PRECISION_MIXED) {
    return "unknown precision (MMX_PRECISION_*)";
  }
  return nullptr;
}

const char* optionsRefusal(const mmx_gn_options& o, bool checkStepRule) {
  if (o.max_iterations < 0 || o.min_iterations < 0) {
    return "iteration counts must be >= 0";
  }
  if (checkStepRule && o.step_rule != MMX_STEP_GN_FIXED_LAMBDA && o.step_rule != MMX_STEP_LM_SCHEDULE && o.step_rule != MMX_STEP_TRUST_REGION) {
    return "unknown step_rule";
  }
  if (o.do_line_search != MMX_LINE_SEARCH_NONE && o.do_line_search != MMX_LINE_SEARCH_GAUSS_NEWTON && o.do_line_search != MMX_LINE_SEARCH_DIRECTIONAL) {
    return "unknown do_line_search rule";
  }
  return nullptr;
}

const char* waveRefusal(const SolveFacts& f, const mmx_gn_options& o, bool frames) {
  if (f.J > MMX_WAVE_MAX_JOINTS) {
    return "MMX_ROUTE_WAVE: more than MMX_WAVE_MAX_JOINTS (64) joints";
  }
  if (f.n > MMX_WAVE_MAX_SOLVED) {
    return "MMX_ROUTE_WAVE: more than MMX_WAVE_MAX_SOLVED (32) solved parameters";
  }
  if (f.n <= 0 || f.U <= 0) {
    return "MMX_ROUTE_WAVE: no solved parameter, or no position / orientation constraint";
  }
  if (f.U > MMX_WAVE_MAX_UNITS) {
    return "MMX_ROUTE_WAVE: more than MMX_WAVE_MAX_UNITS (192) constraint vectors (positions + 3 x orientations)";
  }
  if (f.lossPosType != 0 || f.lossOriType != 0) {
    return "MMX_ROUTE_WAVE: robust losses are outside the route (L2 only)";
  }
  if (f.numBlocks > 0 || f.G > 0 || f.GT > 0) {
    return "MMX_ROUTE_WAVE: further joint-constraint blocks are outside the route";
  }
  if (f.NE > 0) {
    return "MMX_ROUTE_WAVE: ellipsoid limits are outside the route";
  }
  if (f.NL > 0) {
    return "MMX_ROUTE_WAVE: parameter limits are outside the route";
  }
  if (f.hasModel != 0 || f.M > f.rowsJoint) {
    return "MMX_ROUTE_WAVE: the model-parameter prior is outside the route";
  }
  if (f.instanceParents) {
    return "MMX_ROUTE_WAVE: per-instance constraint parents are outside the route";
  }
  if (o.step_rule != MMX_STEP_GN_FIXED_LAMBDA) {
    return "MMX_ROUTE_WAVE: only MMX_STEP_GN_FIXED_LAMBDA (not the LM schedule, not the trust region)";
  }
  if ((frames ? f.waveFramesLdsBytes : f.waveLdsBytes) > kPlanLdsBudget) { // (frames: one more parameter vector per wave)
    return "MMX_ROUTE_WAVE: the parameter vector does not fit a wave's share of LDS";
  }
  return nullptr;
}

const char* gradientRefusal(const SolveFacts& f) {
  if (f.numBlocks > 0 || f.G > 0) {
    return "mmx_eval_gradient: further joint-constraint blocks are outside the matrix-free kernel (mmx_eval_jacobian takes them)";
  }
  if (f.NE > 0) {
    return "mmx_eval_gradient: ellipsoid limits are outside the matrix-free kernel (mmx_eval_jacobian takes them)";
  }
  if (f.instanceParents) {
    return "mmx_eval_gradient: per-instance constraint parents are outside the matrix-free kernel (mmx_eval_jacobian takes them)";
  }
  if (f.U <= 0 || f.n <= 0) {
    return "mmx_eval_gradient: no position / orientation constraint, or no solved parameter";
  }
  if (f.gradientLdsBytes > kPlanLdsBudget - 64) {
    return "mmx_eval_gradient: the rig's tables do not fit the kernel's LDS budget (160 KB)";
  }
  return nullptr;
}

const char* stateBackwardRefusal(size_t ldsBytes) {
  if (ldsBytes > kPlanLdsBudget - 64) {
    return "mmx_eval_skeleton_state_backward: the rig's tables do not fit the kernel's LDS budget (160 KB)";
  }
  return nullptr;
}

SolvePlan planSolveF64(const SolveFacts& f, const mmx_gn_options& o) {
  if (const char* why = optionsRefusal(o, true)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, why);
  }
  if (const char* why = f64Refusal(f)) {
    return refuse(MMX_ERR_UNSUPPORTED, why);
  }
  return oneStage(stageOf(SolveStageKind::Double, SolveStageSelect::All, MMX_ROUTE_AUTO));
}

SolvePlan planSolve(const SolveFacts& f, const mmx_gn_options& o) {
  if (const char* why = preHandleRefusal(o, f.stepHistory)) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, why);
  }
  if (o.precision == MMX_PRECISION_F32) {
    return planSingle(f, o, false);
  }
  if (f.route == MMX_ROUTE_WAVE) {
    return refuse(MMX_ERR_UNSUPPORTED, "MMX_ROUTE_WAVE: only MMX_PRECISION_F32 (not F64 / AUTO / MIXED)");
  }
  const bool mixedOk = mixedUsable(f, o);
  const bool mixedAlone = o.precision == MMX_PRECISION_MIXED && mixedOk;
  if (f.parameterHistory && !mixedAlone) {
    return refuse(MMX_ERR_UNSUPPORTED, "parameter_history is single precision's (MMX_PRECISION_F32) and the mixed-precision instantiation's: the double instantiation does not record it");
  }
  if (mixedAlone) {
    if (const char* why = optionsRefusal(o, true)) { // (the trust region, which the instantiation does not carry, is outside mixedUsable)
      return refuse(MMX_ERR_INVALID_ARGUMENT, why);
    }
    SolveStage s = stageOf(SolveStageKind::Mixed, SolveStageSelect::All, MMX_ROUTE_FUSED);
      return oneStage(s);
  }
  // MMX_PRECISION_F64, MIXED outside the mixed instantiation's scope, and AUTO with the trust region: the rule's elements are
  // marginal by construction (it starts from lambda = 1e-10, the factor's damping floor engages on every element, and its
  // Newton updates of lambda divide two fp32 quadratic forms: the single-precision instantiation is held to 1e-4,
  // tests/test_gpu_trust_region.py) and the mixed instantiation does not carry the rule -- the policy's answer is the double
  // kernel for every element, without a single-precision pass thrown away first
  if (o.precision != MMX_PRECISION_AUTO || o.step_rule == MMX_STEP_TRUST_REGION) {
    return planSolveF64(f, o);
  }
  // MMX_PRECISION_AUTO: single, then mixed on the elements the single pass marked (where the mixed instantiation takes the
  // problem), then double on what is still marked.  Whatever can refuse in a later stage is settled before the first runs.
  if (const char* why = f64Refusal(f)) {
    return refuse(MMX_ERR_UNSUPPORTED, why);
  }
  SolvePlan p = planSingle(f, o, mixedOk);
  if (p.code != MMX_OK) {
    return p;
  }
  if (mixedOk) {
    p.stages[p.numStages++] = stageOf(SolveStageKind::Mixed, SolveStageSelect::SingleSuspects, MMX_ROUTE_FUSED);
  }
  p.stages[p.numStages++] = stageOf(SolveStageKind::Double, mixedOk ? SolveStageSelect::MixedSuspects : SolveStageSelect::SingleSuspects, MMX_ROUTE_AUTO);
  return p;
}

SolvePlan planSolveFrames(const SolveFacts& f, const mmx_gn_options& o, int32_t batch, int32_t numFrames) {
  if (numFrames < 1 || batch % numFrames != 0) {
    return refuse(MMX_ERR_INVALID_ARGUMENT, "mmx_solve_frames: num_frames must be >= 1 and divide the problem's batch (num_frames x sequences instances, frame-major)");
  }
  if (const char* why = optionsRefusal(o, false)) { // (the step rule is the wave route's to refuse)
    return refuse(MMX_ERR_INVALID_ARGUMENT, why);
  }
  if (o.precision != MMX_PRECISION_F32) {
    return refuse(MMX_ERR_UNSUPPORTED, "mmx_solve_frames runs on MMX_ROUTE_WAVE: only MMX_PRECISION_F32 (not F64 / AUTO / MIXED)");
  }
  if (f.route != MMX_ROUTE_AUTO && f.route != MMX_ROUTE_WAVE) {
    return refuse(MMX_ERR_UNSUPPORTED, "mmx_solve_frames runs on the one-wavefront route only: the handle's route is pinned to another (MMX_ROUTE_AUTO or MMX_ROUTE_WAVE)");
  }
  if (const char* why = waveRefusal(f, o, true)) {
    return refuse(MMX_ERR_UNSUPPORTED, why);
  }
  return oneStage(stageOf(SolveStageKind::Single, SolveStageSelect::All, MMX_ROUTE_WAVE));
}

} // namespace mmx
