// The solver's step and stopping rules (momentum_amd/csrc/mmx_solver_rules.hpp) against a transcription of the expressions the
// solve kernels spelled out at every site before the header existed, bit for bit, over a generated grid plus the edge cases
// of every rule.  A stand-alone program: the header, nothing else, no GPU.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all test_solver_rules.cpp
// -DMMX_RULES_HEADER='"<path>"' compiles it against another copy of the header: tests/test_solver_rules_host.py runs it that
// way against mutants of the header (one comparison flipped or one constant changed each) and expects every one to fail.
//
// namespace parent repeats, with their operand order, casts and float / double placement, the expressions of mmx_kernels.hip,
// mmx_fused.hip, mmx_f64.hip and mmx_wave.hip as they stood in the commit before the header (the site is named at each).
// They are the specification: they are not edited to make this test pass.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#ifndef MMX_RULES_HEADER
#define MMX_RULES_HEADER "../../momentum_amd/csrc/mmx_solver_rules.hpp"
#endif
#include MMX_RULES_HEADER

namespace parent {
// mmx_kernels.hip:1637, 2427, 3503; mmx_fused.hip:2726; mmx_f64.hip:1739; mmx_wave.hip:693
bool converged(double last, double e, float threshold) {
  return fabs(last - e) / (fabs(e) + double(FLT_MIN)) <= double(threshold) * double(FLT_EPSILON);
}
bool stops(int iteration, int minIterations, double last, double e, float threshold) {
  const bool converged = fabs(last - e) / (fabs(e) + double(FLT_MIN)) <= double(threshold) * double(FLT_EPSILON);
  return iteration >= minIterations && converged;
}
// mmx_fused.hip:2611, mmx_kernels.hip:3346 | mmx_fused.hip:2500, mmx_f64.hip:1677
float lmRho(double curError, double eNew, float predicted) { return predicted > 0.f ? float((curError - eNew) / double(predicted)) : -1.f; }
double lmRho(double curError, double eNew, double predicted) { return predicted > 0.0 ? (curError - eNew) / predicted : -1.0; }
// mmx_fused.hip:2574, mmx_kernels.hip:3303 | mmx_f64.hip:1657
float trRho(double curError, double eNew, float predicted) { return float((curError - eNew) / double(predicted)); }
double trRho(double curError, double eNew, double predicted) { return (curError - eNew) / predicted; }
// mmx_fused.hip:2625, mmx_kernels.hip:3358
float lmNext(float lambda, float rho, float lmUp, float lmDown, float lmLambdaMin, float lmLambdaMax) {
  if (!(rho >= 0.25f)) {
    lambda = fminf(lambda * lmUp, lmLambdaMax);
  } else if (rho > 0.75f) {
    lambda = fmaxf(lambda * lmDown, lmLambdaMin);
  }
  return lambda;
}
// mmx_fused.hip:2514, mmx_f64.hip:1686
double lmNext(double lambda, double rho, float lmUp, float lmDown, float lmLambdaMin, float lmLambdaMax) {
  if (!(rho >= 0.25)) {
    lambda = fmin(lambda * double(lmUp), double(lmLambdaMax));
  } else if (rho > 0.75) {
    lambda = fmax(lambda * double(lmDown), double(lmLambdaMin));
  }
  return lambda;
}
// mmx_f64.hip:1697 (mmx_fused.hip:2636 and mmx_kernels.hip:3228, the float form, were unreachable and are gone)
double lmRaised(double lambda, float lmUp, float lmLambdaMax) { return fmin(lambda * double(lmUp), double(lmLambdaMax)); }
float lmRaised(float lam, float lmUp, float lmLambdaMax) { return fminf(lam * lmUp, lmLambdaMax); }
// mmx_fused.hip:2662, mmx_wave.hip:660, mmx_kernels.hip:3385
bool armijoF(int doLineSearch, double curError, double eNew, float scale, float scaledError, double gd) {
  return (curError - eNew) >= (doLineSearch == 2 ? double(1e-4f * scale) * gd : double(scale * scaledError));
}
// mmx_fused.hip:2541 (the mixed instantiation: scaledError in double)
bool armijoMixed(int doLineSearch, double curError, double eNew, float scale, double scaledError, double gd) {
  return (curError - eNew) >= (doLineSearch == 2 ? double(1e-4f * scale) * gd : double(scale) * scaledError);
}
// mmx_f64.hip:1708, 1720
bool armijoF64Directional(double curError, double eNew, float alpha, double gd) { return (curError - eNew) >= double(1e-4f * alpha) * gd; }
bool armijoF64(double curError, double eNew, double scale, double scaledError) { return (curError - eNew) >= scale * scaledError; }
// mmx_fused.hip:2451, mmx_kernels.hip:3453 | mmx_f64.hip:1624
bool trGradient(int newton, float dg, double curError) { return newton == 0 && 2.f * dg < FLT_EPSILON * (1.f + float(curError)); }
bool trGradient(int newton, double dg, double curError) { return newton == 0 && 2.0 * dg < double(FLT_EPSILON) * (1.0 + curError); }
// mmx_fused.hip:2455, mmx_kernels.hip:3455 | mmx_f64.hip:1628
bool trNewton(int newton, float dn2, float radius) { return newton < 3 && sqrtf(dn2) >= 1.05f * radius; }
bool trNewton(int newton, double dn2, double trRadius) { return newton < 3 && sqrt(dn2) >= 1.05 * trRadius; }
// mmx_fused.hip:2467-2469, mmx_kernels.hip:3470-3472 | mmx_f64.hip:1636-1638
bool trQ2(float q2) { return q2 >= FLT_EPSILON; }
bool trQ2(double q2) { return q2 >= double(FLT_EPSILON); }
float trDelta(float dn2, float q2, float radius) {
  const float pn = sqrtf(dn2);
  return (dn2 / q2) * ((pn - radius) / radius);
}
double trDelta(double dn2, double q2, double trRadius) {
  const double pn = sqrt(dn2);
  return (dn2 / q2) * ((pn - trRadius) / trRadius);
}
// mmx_fused.hip:2573, mmx_kernels.hip:3302 | mmx_f64.hip:1656
float trPredicted(float dg, float mu, float dn2) { return dg + (mu - 1e-20f) * dn2; }
double trPredicted(double dg, double mu, double dn2) { return dg + (mu - 1e-20) * dn2; }
// mmx_fused.hip:2575-2579, mmx_kernels.hip:3305-3309 (lambda > 0 always holds there: it starts at 1e-10)
float trRadius(float rho, float radius) {
  if (rho < 0.25f) {
    radius = 0.25f * radius;
  } else if (rho > 0.75f) {
    radius = fminf(2.f * radius, 10.f);
  }
  return radius;
}
// mmx_f64.hip:1658-1662
double trRadius(double rho, double trRadius, double lam) {
  if (rho < 0.25) {
    trRadius = 0.25 * trRadius;
  } else if (rho > 0.75 && lam > 0.0) {
    trRadius = fmin(2.0 * trRadius, 10.0);
  }
  return trRadius;
}
// mmx_kernels.hip:909-917, 1599-1609, 2618-2628; mmx_fused.hip:2416-2426 and mmx_wave.hip:629-637 (which spell the literals):
// 0 = undo and stop, 1 = keep and stop, 2 = keep, another step may follow
constexpr float kRefineTol2 = 1e-6f;
constexpr float kRefineMax2 = 0.25f;
int refine(float corr2, float step2, float prevCorr2) {
  if (corr2 > kRefineMax2 * step2 || corr2 > prevCorr2) {
    return 0;
  }
  if (!(corr2 > kRefineTol2 * step2)) {
    return 1;
  }
  return 2;
}
int refineLiterals(float corr2, float step2, float prevCorr2) {
  if (corr2 > 0.25f * step2 || corr2 > prevCorr2) {
    return 0;
  }
  if (!(corr2 > 1e-6f * step2)) {
    return 1;
  }
  return 2;
}
// mmx_kernels.hip:3150-3157 (the finish stage of the wide route: no comparison with the round before)
int refineFinish(float corr2, float step2) {
  bool again = corr2 > kRefineTol2 * step2;
  bool undo = false;
  if (corr2 > kRefineMax2 * step2) {
    undo = true;
    again = false;
  }
  return undo ? 0 : (again ? 2 : 1);
}
// mmx_device.hpp:42, 72-73; mmx_fused.hip:2732, 2772, mmx_kernels.hip:3572
constexpr float kPivotFloor = 3.814697265625e-6f;
constexpr float kPrecisionGain = 0.042f;
constexpr float kPivotFloorOrOne = kPivotFloor > 0.f ? kPivotFloor : 1.f;
float estimate(float wS) { return kPrecisionGain * FLT_EPSILON * wS / kPivotFloorOrOne; }
bool suspect(float est, float precisionBound) { return !(est <= precisionBound); }
// mmx_fused.hip:2773, mmx_wave.hip:728 | mmx_f64.hip:1791
int32_t status(bool bad, int32_t flags) { return bad ? 1 : flags; }
int32_t statusF64(bool bad, int32_t flags, bool listMode, int32_t firstPass) { return (bad ? 1 : flags) | (listMode ? ((firstPass & 8) | 16) : 0); }
} // namespace parent

namespace {

long checks = 0;

template <class T>
uint64_t bits(T v) {
  uint64_t u = 0;
  static_assert(sizeof(T) <= sizeof(u), "");
  std::memcpy(&u, &v, sizeof(T));
  return u;
}
uint64_t bits(bool v) { return v ? 1 : 0; }

#define SAME(a, b)                                                                                                           \
  do {                                                                                                                       \
    ++checks;                                                                                                                \
    if (bits(a) != bits(b)) {                                                                                                \
      std::printf("FAILED %s:%d: %s = %.17g, %s = %.17g\n", __FILE__, __LINE__, #a, double(a), #b, double(b));                 \
      std::exit(1);                                                                                                          \
    }                                                                                                                        \
  } while (0)

// a deterministic generator (no <random>: the same grid on every platform)
struct Rng {
  uint64_t s = 0x9E3779B97F4A7C15ull;
  uint64_t next() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return s;
  }
  double unit() { return double(next() >> 11) * (1.0 / 9007199254740992.0); }
  double log10Uniform(double lo, double hi) { return std::pow(10.0, lo + (hi - lo) * unit()); } // 10^[lo, hi)
  double signedLog(double lo, double hi) { return (next() & 1 ? -1.0 : 1.0) * log10Uniform(lo, hi); }
};

const float kNaNf = std::numeric_limits<float>::quiet_NaN();
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const float kInff = std::numeric_limits<float>::infinity();

int verdict(float corr2, float step2, float prevCorr2) {
  return mmx::refineUndo(corr2, step2, prevCorr2) ? 0 : (mmx::refineAgain(corr2, step2) ? 2 : 1);
}

void testConverged(Rng& rng) {
  std::vector<double> es = {0.0, 1.0, 1e-30, 1e-300, 3.5, 1e6, DBL_MAX, double(FLT_MIN), 2e-44, 1e-44, 1.4e-45, kNaN};
  std::vector<float> ths = {0.f, 1.f, 10.f, 100.f, 1e4f, 8388608.f, 1e10f, kNaNf};
  for (int i = 0; i < 40; ++i) {
    es.push_back(rng.log10Uniform(-12, 8));
  }
  for (double e : es) {
    std::vector<double> lasts = {DBL_MAX, e, 0.0, 2e-44, 1e-44, 1.4e-45, kNaN}; // the first iteration; no change at all
    for (float th : ths) {
      // ... and `last` on both sides of the rule's boundary |last - e| = th eps (|e| + FLT_MIN), to the ulp
      const double edge = (std::fabs(e) + double(FLT_MIN)) * double(th) * double(FLT_EPSILON);
      for (double f : {0.0, 0.5, 0.999999, 1.0, 1.000001, 2.0}) {
        lasts.push_back(e + f * edge);
        lasts.push_back(e - f * edge);
      }
      lasts.push_back(std::nextafter(e + edge, DBL_MAX));
      lasts.push_back(std::nextafter(e + edge, -DBL_MAX));
    }
    for (double last : lasts) {
      for (float th : ths) {
        SAME(mmx::solveConverged(last, e, th), parent::converged(last, e, th));
        for (int it = 0; it < 4; ++it) {
          for (int minIt = 0; minIt < 4; ++minIt) {
            SAME(mmx::solveStops(it, minIt, last, e, th), parent::stops(it, minIt, last, e, th));
          }
        }
      }
    }
  }
}

void testLm(Rng& rng) {
  std::vector<double> preds = {0.0, -0.0, -1.0, -1e-30, 1e-30, 0.5, 1.0, 3.0, kNaN, double(kInff)};
  std::vector<double> curs = {0.0, 1.0, 2.5, 1e-8, 1e8, kNaN};
  for (int i = 0; i < 30; ++i) {
    preds.push_back(rng.signedLog(-10, 6));
    curs.push_back(rng.log10Uniform(-10, 8));
  }
  for (double cur : curs) {
    for (double p : preds) {
      for (double f : {-1.0, 0.0, 0.2499999, 0.25, 0.2500001, 0.5, 0.75, 0.7500001, 1.0, 2.0}) { // the actual decrease as a share of the predicted one
        const double eNew = cur - f * p;
        SAME(mmx::lmGainRatio(cur, eNew, float(p)), parent::lmRho(cur, eNew, float(p)));
        SAME(mmx::lmGainRatio(cur, eNew, p), parent::lmRho(cur, eNew, p));
        SAME(mmx::gainRatio(cur, eNew, float(p)), parent::trRho(cur, eNew, float(p)));
        SAME(mmx::gainRatio(cur, eNew, p), parent::trRho(cur, eNew, p));
      }
    }
  }
  // rho exactly at 0.25 and 0.75, next to them, NaN; lambda at, inside and outside both clamps
  std::vector<double> rhos = {0.25, 0.75, std::nextafter(0.25, 0.0), std::nextafter(0.25, 1.0), std::nextafter(0.75, 0.0), std::nextafter(0.75, 1.0),
                              double(std::nextafterf(0.25f, 0.f)), double(std::nextafterf(0.75f, 1.f)), -1.0, 0.0, 0.5, 1.0, 100.0, kNaN, double(kInff), -double(kInff)};
  const float lo = 1e-7f, hi = 1e3f;
  std::vector<double> lams = {double(lo), double(hi), double(lo) * 1.5, double(hi) / 1.5, double(lo) / 3.0, double(hi) * 3.0, 0.05, 0.0, kNaN};
  for (int i = 0; i < 20; ++i) {
    rhos.push_back(rng.signedLog(-3, 2));
    lams.push_back(rng.log10Uniform(-9, 5));
  }
  for (double lam : lams) {
    for (double rho : rhos) {
      for (float up : {2.f, 10.f, 1.f}) {
        for (float down : {0.5f, 0.1f, 1.f / 3.f}) {
          SAME(mmx::lmNextLambda(float(lam), float(rho), up, down, lo, hi), parent::lmNext(float(lam), float(rho), up, down, lo, hi));
          SAME(mmx::lmNextLambda(lam, rho, double(up), double(down), double(lo), double(hi)), parent::lmNext(lam, rho, up, down, lo, hi));
        }
        SAME(mmx::lmRaisedLambda(lam, double(up), double(hi)), parent::lmRaised(lam, up, hi));
        SAME(mmx::lmRaisedLambda(float(lam), up, hi), parent::lmRaised(float(lam), up, hi));
      }
    }
  }
}

void testArmijo(Rng& rng) {
  std::vector<double> curs = {0.0, 1.0, 1e-8, 1e8, 3.75, kNaN};
  std::vector<double> gds = {0.0, 1.0, -1.0, 1e-6, 1e6, kNaN};
  for (int i = 0; i < 12; ++i) {
    curs.push_back(rng.log10Uniform(-10, 8));
    gds.push_back(rng.signedLog(-8, 8));
  }
  for (double cur : curs) {
    const float scaledF = 1e-3f * float(cur); // (the sites' scaledError, single and double)
    const double scaledD = 1e-3 * cur;
    for (double gd : gds) {
      float scale = 1.f;
      for (int ls = 0; ls < 10; ++ls, scale *= 0.5f) {
        for (int rule : {1, 2}) {
          // the decrease at the bound of the rule in force, next to it, and away from it
          const double bound = rule == 2 ? double(1e-4f * scale) * gd : double(scale * scaledF);
          for (double dec : {bound, std::nextafter(bound, DBL_MAX), std::nextafter(bound, -DBL_MAX), double(scale) * scaledD, 0.0, -bound, 2.0 * bound, kNaN}) {
            const double eNew = cur - dec;
            SAME(mmx::armijoAccepts(rule, cur, eNew, scale, scaledF, gd), parent::armijoF(rule, cur, eNew, scale, scaledF, gd));
            SAME(mmx::armijoAccepts(rule, cur, eNew, scale, scaledD, gd), parent::armijoMixed(rule, cur, eNew, scale, scaledD, gd));
          }
        }
        const double b2 = double(1e-4f * scale) * gd, b1 = double(scale) * scaledD;
        for (double dec : {b2, b1, std::nextafter(b2, DBL_MAX), std::nextafter(b1, DBL_MAX), std::nextafter(b2, -DBL_MAX), std::nextafter(b1, -DBL_MAX), 0.0, kNaN}) {
          const double eNew = cur - dec;
          SAME(mmx::armijoAccepts(MMX_LINE_SEARCH_DIRECTIONAL, cur, eNew, scale, 0.0, gd), parent::armijoF64Directional(cur, eNew, scale, gd));
          SAME(mmx::armijoAccepts(MMX_LINE_SEARCH_GAUSS_NEWTON, cur, eNew, double(scale), scaledD, 0.0), parent::armijoF64(cur, eNew, double(scale), scaledD));
        }
      }
    }
  }
}

void testTrust(Rng& rng) {
  static_assert(mmx::kTrustMaxTrials == 10, "rules constant differs from the sites: trust_region_qr.cpp:157; mmx_fused.hip:2586, mmx_kernels.hip:3322, mmx_f64.hip:1580");
  std::vector<double> curs = {0.0, 1.0, 1e-8, 1e8, kNaN};
  for (int i = 0; i < 10; ++i) {
    curs.push_back(rng.log10Uniform(-10, 8));
  }
  for (double cur : curs) {
    // dg on both sides of eps (1 + e) / 2
    const double edge = 0.5 * double(FLT_EPSILON) * (1.0 + cur);
    for (double dg : {0.0, -1.0, edge, edge * 0.999, edge * 1.001, double(std::nextafterf(float(edge), 0.f)), double(std::nextafterf(float(edge), 1e30f)), 1.0, kNaN}) {
      for (int newton = 0; newton < 3; ++newton) {
        SAME(mmx::trustGradientTooSmall(newton, float(dg), cur), parent::trGradient(newton, float(dg), cur));
        SAME(mmx::trustGradientTooSmall(newton, dg, cur), parent::trGradient(newton, dg, cur));
      }
    }
  }
  std::vector<double> radii = {10.0, 1.0, 0.25, 1e-3, 5.0, 5.000001, 9.999999, 20.0, kNaN}; // the cap of 10, half of it, past it
  std::vector<double> dn2s = {0.0, 1.0, 1e-12, 1e12, kNaN};
  for (int i = 0; i < 12; ++i) {
    radii.push_back(rng.log10Uniform(-4, 1));
    dn2s.push_back(rng.log10Uniform(-10, 6));
  }
  const double eps = double(FLT_EPSILON);
  std::vector<double> q2s = {eps, double(std::nextafterf(FLT_EPSILON, 0.f)), double(std::nextafterf(FLT_EPSILON, 1.f)), std::nextafter(eps, 0.0), std::nextafter(eps, 1.0), 0.0, 1.0, 1e-3, 1e6, -1.0, kNaN};
  for (double r : radii) {
    std::vector<double> d = dn2s;
    for (double f : {1.05, 1.0499999, 1.0500001, 1.0, 2.0}) { // |step| on both sides of 1.05 r
      d.push_back((f * r) * (f * r));
      d.push_back(double(float(f * r) * float(f * r)));
    }
    for (double dn2 : d) {
      for (int newton = 0; newton < 8; ++newton) {
        SAME(mmx::trustWantsNewton(newton, float(dn2), float(r)), parent::trNewton(newton, float(dn2), float(r)));
        SAME(mmx::trustWantsNewton(newton, dn2, r), parent::trNewton(newton, dn2, r));
      }
      for (double q2 : q2s) {
        SAME(mmx::trustNewtonDefined(float(q2)), parent::trQ2(float(q2)));
        SAME(mmx::trustNewtonDefined(q2), parent::trQ2(q2));
        SAME(mmx::trustDeltaLambda(float(dn2), float(q2), float(r)), parent::trDelta(float(dn2), float(q2), float(r)));
        SAME(mmx::trustDeltaLambda(dn2, q2, r), parent::trDelta(dn2, q2, r));
      }
      for (double mu : {1e-20, 0.0, 1e-10, 2e-20, 1.5e-20, 1e-3, 1.0, kNaN}) {
        for (double dg : {0.0, 1.0, -1.0, 1e-20, 1e-6, kNaN}) {
          SAME(mmx::trustPredicted(float(dg), float(mu), float(dn2)), parent::trPredicted(float(dg), float(mu), float(dn2)));
          SAME(mmx::trustPredicted(dg, mu, dn2), parent::trPredicted(dg, mu, dn2));
        }
      }
    }
    for (double rho : {0.25, 0.75, std::nextafter(0.25, 0.0), std::nextafter(0.25, 1.0), std::nextafter(0.75, 0.0), std::nextafter(0.75, 1.0), double(std::nextafterf(0.25f, 0.f)),
                       double(std::nextafterf(0.75f, 1.f)), -1.0, 0.0, 0.5, 1.0, 1e3, kNaN, double(kInff), -double(kInff)}) {
      SAME(mmx::trustNextRadius(float(rho), float(r), true), parent::trRadius(float(rho), float(r)));
      for (double lam : {1e-10, 0.0, -1.0, 3.0, kNaN}) {
        SAME(mmx::trustNextRadius(rho, r, lam > 0.0), parent::trRadius(rho, r, lam));
      }
    }
  }
}

void testRefine(Rng& rng) {
  static_assert(mmx::kRefineTol2 == parent::kRefineTol2 && mmx::kRefineMax2 == parent::kRefineMax2, "rules constant differs from the sites: mmx_kernels.hip:910, 917");
  std::vector<float> step2s = {0.f, 1.f, 1e-12f, 1e12f, 3.f, kNaNf, kInff};
  for (int i = 0; i < 30; ++i) {
    step2s.push_back(float(rng.log10Uniform(-12, 8)));
  }
  for (float step2 : step2s) {
    std::vector<float> corr2s = {0.f, step2, kNaNf, kInff, FLT_MAX};
    for (float t : {parent::kRefineTol2 * step2, parent::kRefineMax2 * step2}) { // corr2 equal to each threshold times step2, and its neighbours
      corr2s.push_back(t);
      corr2s.push_back(std::nextafterf(t, 0.f));
      corr2s.push_back(std::nextafterf(t, kInff));
    }
    for (int i = 0; i < 6; ++i) {
      corr2s.push_back(step2 * float(rng.log10Uniform(-9, 1)));
    }
    for (float corr2 : corr2s) {
      for (float prev : {FLT_MAX, corr2, std::nextafterf(corr2, 0.f), std::nextafterf(corr2, kInff), 0.f, 1e-3f * step2, kNaNf, kInff}) {
        SAME(verdict(corr2, step2, prev), parent::refine(corr2, step2, prev));
        SAME(verdict(corr2, step2, prev), parent::refineLiterals(corr2, step2, prev));
      }
      SAME(mmx::refineDiverges(corr2, step2) ? 0 : (mmx::refineAgain(corr2, step2) ? 2 : 1), parent::refineFinish(corr2, step2)); // how choleskyFinishTiledKernel asks
    }
  }
}

void testPrecision(Rng& rng) {
  std::vector<float> ws = {0.f, 1.f, parent::kPivotFloor, 1e-3f, 0.5f, kNaNf, kInff, FLT_MIN, FLT_MAX};
  for (int i = 0; i < 200; ++i) {
    ws.push_back(float(rng.log10Uniform(-8, 1)));
  }
  for (float w : ws) {
    const float est = parent::estimate(w);
    SAME(mmx::precisionEstimate(parent::kPrecisionGain, w, parent::kPivotFloorOrOne), est);
    for (float bound : {est, std::nextafterf(est, 0.f), std::nextafterf(est, kInff), 1e-5f, 0.f, -1.f, kNaNf, kInff}) {
      SAME(mmx::precisionSuspect(est, bound), parent::suspect(est, bound));
    }
  }
}

void testStatus() {
  // every combination of the bits (a superset of what the kernels produce: NOT_PD | DAMPING_FLOORED | PRECISION_SUSPECT | MIXED
  // from the single and mixed passes, NOT_PD from the double one, NONFINITE alone), as the pass's own word and as the first pass's
  for (int32_t own = 0; own < 64; ++own) {
    for (int bad = 0; bad < 2; ++bad) {
      SAME(mmx::solveStatus(bad != 0, own), parent::status(bad != 0, own));
      for (int32_t first = 0; first < 64; ++first) {
        SAME(mmx::escalatedStatus(mmx::solveStatus(bad != 0, own), first), parent::statusF64(bad != 0, own, true, first));
        SAME(mmx::solveStatus(bad != 0, own), parent::statusF64(bad != 0, own, false, first));
      }
    }
  }
  static_assert(MMX_SOLVE_NONFINITE == 1 && MMX_SOLVE_NOT_PD == 2 && MMX_SOLVE_DAMPING_FLOORED == 4 && MMX_SOLVE_PRECISION_SUSPECT == 8 && MMX_SOLVE_ESCALATED_F64 == 16 && MMX_SOLVE_MIXED == 32, "the literals of the sites");
  static_assert(MMX_STEP_GN_FIXED_LAMBDA == 0 && MMX_STEP_LM_SCHEDULE == 1 && MMX_STEP_TRUST_REGION == 2, "the literals of the sites");
  static_assert(MMX_LINE_SEARCH_NONE == 0 && MMX_LINE_SEARCH_GAUSS_NEWTON == 1 && MMX_LINE_SEARCH_DIRECTIONAL == 2, "the literals of the sites");
}

} // namespace

int main() {
  Rng rng;
  testConverged(rng);
  testLm(rng);
  testArmijo(rng);
  testTrust(rng);
  testRefine(rng);
  testPrecision(rng);
  testStatus();
  std::printf("%ld comparisons\nOK\n", checks);
  return 0;
}
