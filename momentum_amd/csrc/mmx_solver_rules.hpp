// mmx_solver_rules.hpp -- the solver's scalar decisions, once, for every solve route: SolverT::solve's stopping rule, the LM
// schedule, both backtracking rules, TrustRegionQRT's step rule, refinement acceptance, the precision estimate, the status word.
// Pure functions of scalars (no HIP include, no LDS, no thread index); tests/cpp/test_solver_rules.cpp holds each, bit for bit,
// against the expressions the kernels spelled out before.  An expression here is TEXTUALLY the kernels' (operand order, casts,
// float / double placement): another text contracts other multiply-adds.  oracle/mmx_oracle.hpp does not include this header.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/mmx.h"

#if defined(__HIPCC__)
#define MMX_RULE __host__ __device__ inline __attribute__((always_inline)) // (= __forceinline__, which only the HIP runtime header defines)
#else
#define MMX_RULE inline
#endif

namespace mmx {

// (the float instantiations' constants are the kernels' float literals)
static_assert(float(1.05) == 1.05f && float(1e-20) == 1e-20f, "T(literal) must be the float literal");

MMX_RULE float ruleSqrt(float x) { return sqrtf(x); }
MMX_RULE double ruleSqrt(double x) { return sqrt(x); }
MMX_RULE float ruleMin(float a, float b) { return fminf(a, b); }
MMX_RULE double ruleMin(double a, double b) { return fmin(a, b); }
MMX_RULE float ruleMax(float a, float b) { return fmaxf(a, b); }
MMX_RULE double ruleMax(double a, double b) { return fmax(a, b); }

// ---- SolverT::solve (momentum/solver/solver.cpp:96-119): the relative change of the error against threshold x eps;
// `last` is DBL_MAX in the first iteration (:84-85)
MMX_RULE bool solveConverged(double last, double e, float threshold) {
  return fabs(last - e) / (fabs(e) + double(FLT_MIN)) <= double(threshold) * double(FLT_EPSILON);
}
MMX_RULE bool solveStops(int it, int minIterations, double last, double e, float threshold) {
  const bool converged = solveConverged(last, e, threshold);
  return it >= minIterations && converged;
}

// ---- the LM gain-ratio schedule, the lambda form of TrustRegionQRT's radius rule (momentum/character_solver/
// trust_region_qr.cpp:244-268): rho = actual / predicted decrease (a model that predicts none counts as a rejected step);
// rho below 0.25 (or NaN) raises the damping, above 0.75 lowers it, both clamped
template <class T>
MMX_RULE T gainRatio(double curError, double eNew, T predicted) {
  return T((curError - eNew) / double(predicted));
}
template <class T>
MMX_RULE T lmGainRatio(double curError, double eNew, T predicted) {
  return predicted > T(0) ? gainRatio(curError, eNew, predicted) : T(-1);
}
template <class T> // no step could be taken (H not positive definite): the schedule treats it as a rejected one
MMX_RULE T lmRaisedLambda(T lambda, T up, T hi) {
  return ruleMin(lambda * up, hi);
}
template <class T>
MMX_RULE T lmNextLambda(T lambda, T rho, T up, T down, T lo, T hi) {
  if (!(rho >= T(0.25))) {
    lambda = lmRaisedLambda(lambda, up, hi);
  } else if (rho > T(0.75)) {
    lambda = ruleMax(lambda * down, lo);
  }
  return lambda;
}

// ---- backtracking: MMX_LINE_SEARCH_GAUSS_NEWTON, GaussNewtonSolverT::updateParameters (momentum/solver/
// gauss_newton_solver.cpp:283-313: the decrease against scale x scaledError, scaledError = 1e-3 x the error), and
// MMX_LINE_SEARCH_DIRECTIONAL, SubsetGaussNewtonSolverT / GaussNewtonSolverQRT (subset_gauss_newton_solver.cpp:117-142,
// gauss_newton_solver_qr.cpp:126-149: c_1 = 1e-4, kept in float with the step length, against gd = J^T r . delta).
// The single-precision routes hold scale and scaledError in float, the mixed one scaledError in double, the double kernel
// both in double under the first rule and the step length in float under the second, as the reference's instantiations do.
template <class A, class S>
MMX_RULE bool armijoAccepts(int rule, double curError, double eNew, A scale, S scaledError, double gd) {
  return (curError - eNew) >= (rule == MMX_LINE_SEARCH_DIRECTIONAL ? double(1e-4f * scale) * gd : double(scale * scaledError));
}

// ---- TrustRegionQRT::doIteration (momentum/character_solver/trust_region_qr.cpp:52-270)
constexpr int kTrustMaxTrials = 10; // :157: after that many rejected trials the parameters stay (:268-269)
template <class T> // :164 (gradientSub_ = 2 J^T r): not worth a step
MMX_RULE bool trustGradientTooSmall(int newtonIter, T dg, double curError) {
  return newtonIter == 0 && T(2) * dg < T(FLT_EPSILON) * (T(1) + T(curError));
}
template <class T> // :180-181: the step leaves the region and lambda may still take a Newton update
MMX_RULE bool trustWantsNewton(int newtonIter, T dn2, T radius) {
  return newtonIter < 3 && ruleSqrt(dn2) >= T(1.05) * radius;
}
// the Newton update of lambda (Nocedal & Wright eq. 4.44, :191-207), q2 = |q_l|^2 = p_l^T (R^T R)^-1 p_l: none when q2 is
// below eps (:198); lambda only ever grows, so a result <= 0 means none as well (:207).  (The test is a function of its own:
// a "none" folded into the result is a merged value, and `lambda += result` no longer contracts into the multiply-add the
// kernels have.)
template <class T>
MMX_RULE bool trustNewtonDefined(T q2) {
  return q2 >= T(FLT_EPSILON);
}
template <class T>
MMX_RULE T trustDeltaLambda(T dn2, T q2, T radius) {
  const T pn = ruleSqrt(dn2);
  return (dn2 / q2) * ((pn - radius) / radius);
}
// e - model (:240-247), the model being e - 2 g.p + p^T (J^T J + 1e-20 I) p with p^T J^T J p = g.p - mu |p|^2 because
// (J^T J + mu I) p = g
template <class T>
MMX_RULE T trustPredicted(T dg, T mu, T dn2) {
  return dg + (mu - T(1e-20)) * dn2;
}
template <class T> // :256-262 (the reference grows the radius only when lambda > 0)
MMX_RULE T trustNextRadius(T rho, T radius, bool lamPositive) {
  if (rho < T(0.25)) {
    radius = T(0.25) * radius;
  } else if (rho > T(0.75) && lamPositive) {
    radius = ruleMin(T(2) * radius, T(10));
  }
  return radius;
}

// ---- refinement of the step through J: a further refinement step is taken while |correction|^2 > kRefineTol2 |step|^2
// (at most three steps)
constexpr float kRefineTol2 = 1e-6f;
// ... and a correction is only TAKEN when it is a contraction: |correction|^2 <= kRefineMax2 |step|^2, and not larger than
// the correction before it.  With a well-conditioned factor the first correction is 1e-3 ... 1e-5 of the step; where the
// fp32 factor is no preconditioner any more (pivots at rounding level: rank-deficient J with lambda ~ 1e-7) the
// iteration d += M^-1 (g - A d) diverges -- measured in round 3: cfg2 at lambda = 1e-7 ended at a median error of 74 with
// the unguarded refinement, 6 without any (the double solver: 5e-6 ... 16) -- so such a correction is undone and the
// refinement stops.
constexpr float kRefineMax2 = 0.25f;
// The verdict on a correction, in the order the kernels ask: undo it and stop?  Else it is kept -- and may another step follow?
// (Predicates, not one three-valued result: the compiler materialises such a result as an integer in the solve kernels.)
MMX_RULE bool refineDiverges(float corr2, float step2) {
  return corr2 > kRefineMax2 * step2;
}
MMX_RULE bool refineUndo(float corr2, float step2, float prevCorr2) { // prevCorr2: FLT_MAX before the first step
  return refineDiverges(corr2, step2) || corr2 > prevCorr2;
}
MMX_RULE bool refineAgain(float corr2, float step2) {
  return corr2 > kRefineTol2 * step2;
}

// ---- the precision estimate of the single-precision solves from w, the largest weighted kPivotFloor (H_jj + mu) / d_jj
// of the solve (gain = kPrecisionGain, mmx_device.hpp has its calibration), and its test against mmx_gn_options::precision_bound
MMX_RULE float precisionEstimate(float gain, float w, float pivotFloorOrOne) {
  return gain * FLT_EPSILON * w / pivotFloorOrOne;
}
MMX_RULE bool precisionSuspect(float est, float bound) {
  return !(est <= bound);
}

// ---- the status word (MMX_SOLVE_*): a non-finite answer replaces every other bit ...
MMX_RULE int32_t solveStatus(bool nonFinite, int32_t bits) {
  return nonFinite ? MMX_SOLVE_NONFINITE : bits;
}
// ... and an element MMX_PRECISION_AUTO re-solved in double reports the double run's status, why it was taken and that it was
MMX_RULE int32_t escalatedStatus(int32_t own, int32_t firstPass) {
  return own | ((firstPass & MMX_SOLVE_PRECISION_SUSPECT) | MMX_SOLVE_ESCALATED_F64);
}

} // namespace mmx
