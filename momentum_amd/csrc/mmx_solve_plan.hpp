// mmx_solve_plan.hpp -- which kernels a solve call runs, decided before anything is touched (no HIP here, no handle: a pure
// function of plain facts and the caller's options, unit-tested exhaustively on the CPU: tests/cpp/test_solve_plan.cpp).
// mmx_capi.hip gathers the facts from its handle (solveFacts), asks for the plan and either fails with the plan's refusal or
// runs the plan's stages.  The decision order is the table in DESIGN.md section 4 ("The decision, in its order").
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/mmx.h"

namespace mmx {
#pragma GCC visibility push(hidden)

constexpr size_t kPlanLdsBudget = 160 * 1024; // a workgroup's LDS on gfx950
constexpr int32_t kPlanMaxSolved = 2048; // = mmx::kMaxSolved (mmx_kernels.hpp; mmx_capi.hip asserts it)

// What the decision reads.  The sizing functions live in the kernel files and stay there: the facts carry their results.
struct SolveFacts {
  int32_t route = MMX_ROUTE_AUTO; // mmx_tuning::route
  int32_t refineSteps = 3; // refinement steps per iteration (mmx_tuning::max_refinement_steps, resolved)
  bool fusedUsable = false; // the one-launch solve has an instantiation for the problem and its tables fit LDS
  bool treeUsable = false; // the tree kernels (wide route) cover the problem
  bool fusedMixedUsable = false; // the mixed-precision instantiation's LDS budget
  int32_t fusedBlocks = -1; // fusedBlocksFor(n): 16-blocks of the one-launch instantiation, -1 without one
  size_t choleskyStepLdsBytes = 0; // the explicit-Jacobian route's in-LDS Cholesky step
  size_t waveLdsBytes = 0, waveFramesLdsBytes = 0; // the one-wavefront route, plain and with frames
  bool f64Resident = false; // the double kernel keeps J and H in LDS
  size_t f64LdsBytes = 0; // ... its scratch form's budget otherwise
  // the problem's counts
  int32_t J = 0, n = 0 /* one-launch solve list */, solveN = 0 /* explicit-Jacobian solve list */, U = 0, M = 0, rowsJoint = 0;
  int32_t GT = 0, G = 0, NE = 0, NL = 0, numBlocks = 0, hasModel = 0, lossPosType = 0, lossOriType = 0;
  bool instanceParents = false; // per-instance constraint parents are set
  // the optional outputs the caller passed
  bool parameterHistory = false, stepHistory = false;
  size_t gradientLdsBytes = 0; // mmx_eval_gradient's kernel (gradientRefusal reads it; the solve plans do not)
};

enum class SolveStageKind : int32_t { Single, Mixed, Double };
// the elements a stage runs on: all of them, or (MMX_PRECISION_AUTO's later stages) the ones the stage before it marked
enum class SolveStageSelect : int32_t { All, SingleSuspects, MixedSuspects };

struct SolveStage {
  SolveStageKind kind = SolveStageKind::Single;
  SolveStageSelect select = SolveStageSelect::All;
  // Single: MMX_ROUTE_WAVE / FUSED / WIDE / EXPLICIT_JACOBIAN; Mixed: MMX_ROUTE_FUSED; Double: MMX_ROUTE_AUTO (records none)
  int32_t route = MMX_ROUTE_AUTO;
  bool mayAbort = false; // Single under MMX_PRECISION_AUTO: a mixed stage follows, marked elements may leave early
  // the host-driven routes (wide / explicit Jacobian)
  bool wide = false; // the in-LDS Cholesky step does not fit: left-looking factor in HBM
  bool treeRefine = false; // normal equations and refinement through the tree kernels (= the wide route)
  bool wideDiag = false; // ... with the precision estimate
  bool deferred = false; // the step is applied by the step-update kernel (line search, LM schedule, trust region)
  bool schedule = false; // per-instance damping
};

struct SolvePlan {
  int32_t code = MMX_OK; // MMX_OK: run the stages; else the refusal
  const char* message = nullptr;
  int32_t numStages = 0;
  SolveStage stages[3];
};

// The checks mmx_solve* make before they look at the handle (planSolve repeats them first).  Null: none applies.
const char* preHandleRefusal(const mmx_gn_options& o, bool stepHistory);
// The one options check: iteration counts, step rule (mmx_solve_frames leaves that one to the wave route's scope), line-search rule
const char* optionsRefusal(const mmx_gn_options& o, bool checkStepRule);
// MMX_ROUTE_WAVE's scope (table in include/mmx.h): null when the route takes the problem with these options
const char* waveRefusal(const SolveFacts& f, const mmx_gn_options& o, bool frames);
// mmx_eval_gradient's scope (include/mmx.h), in its documented order: null when the matrix-free kernel takes the problem
const char* gradientRefusal(const SolveFacts& f);
// mmx_eval_skeleton_state_backward's one scope rule: its kernel's LDS bytes for the rig (stateBackwardLdsBytes(J, P),
// mmx_kernels.hpp) against the workgroup's budget.  Null: the kernel takes the rig.
const char* stateBackwardRefusal(size_t ldsBytes);

SolvePlan planSolve(const SolveFacts& f, const mmx_gn_options& o); // mmx_solve, mmx_solve_with_history, ..._with_step_history
SolvePlan planSolveF64(const SolveFacts& f, const mmx_gn_options& o); // mmx_solve_f64
SolvePlan planSolveFrames(const SolveFacts& f, const mmx_gn_options& o, int32_t batch, int32_t numFrames); // mmx_solve_frames

#pragma GCC visibility pop
} // namespace mmx
