// GPU smoke test of the nearest-point query in the C++ shell (include/momentum_amd/momentum_amd.hpp, findClosestPoints over
// mmx_closest_points_host): three batch elements of 70 sources against 90 targets (per element, then shared), with and
// without normals and with a finite max_dist, against a double loop written here in double.
//
// Bounds (u = 2^-24): a float32 d2 is within about 5u of the double value, so the chosen target's double distance is within
// (1 + 16u) of the smallest eligible one and the returned dist2 within 8u of the chosen target's; a source is skipped where
// the double minimum sits within 16u of max_dist^2 or a target's dot within 1e-6 of the threshold (none does on these inputs:
// the program counts them and fails above 1 %).
#include <cmath>
#include <cstdio>

#include "momentum_amd/momentum_amd.hpp"

using namespace momentum_amd;

constexpr size_t B = 3, N = 70, M = 90;
constexpr double kU = 1.0 / 16777216.0, kBand = 1e-6;

static float coord(size_t i, double f) {
  return float(std::sin(f * double(i) + 0.3) * 0.8 + 0.1 * std::cos(1.7 * double(i)));
}

static void fill(std::vector<float>& p, std::vector<float>& n, size_t count, double f) {
  p.resize(count * 3), n.resize(count * 3);
  for (size_t i = 0; i < count; ++i) {
    double v[3];
    for (size_t c = 0; c < 3; ++c) {
      p[3 * i + c] = coord(3 * i + c, f);
      v[c] = std::cos(f * 1.3 * double(3 * i + c) + 1.0);
    }
    const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (size_t c = 0; c < 3; ++c) {
      n[3 * i + c] = float(v[c] / len);
    }
  }
}

static int verify(
    const char* what, const ClosestPoints& r, const std::vector<float>& src, const std::vector<float>& tgt, bool shared, const std::vector<float>* sn,
    const std::vector<float>* tn, float maxDist, float minDot) {
  int bad = 0, skipped = 0;
  const double m2 = double(maxDist) * double(maxDist);
  for (size_t b = 0; b < B; ++b) {
    const float* t = tgt.data() + (shared ? 0 : b * M * 3);
    for (size_t s = 0; s < N; ++s) {
      const float* p = src.data() + (b * N + s) * 3;
      double minSure = INFINITY, minMaybe = INFINITY;
      std::vector<double> d(M), dot(M, 1.0);
      for (size_t j = 0; j < M; ++j) {
        d[j] = 0;
        for (size_t c = 0; c < 3; ++c) {
          const double x = double(p[c]) - double(t[3 * j + c]);
          d[j] += x * x;
        }
        if (sn != nullptr) {
          const float* a = sn->data() + (b * N + s) * 3;
          const float* q = tn->data() + (shared ? 0 : b * M * 3) + 3 * j;
          dot[j] = double(a[0]) * q[0] + double(a[1]) * q[1] + double(a[2]) * q[2];
        }
        const double lo = sn ? double(minDot) - kBand : -INFINITY, hi = sn ? double(minDot) + kBand : -INFINITY;
        if (dot[j] >= lo) {
          minMaybe = std::fmin(minMaybe, d[j]);
        }
        if (dot[j] >= hi) {
          minSure = std::fmin(minSure, d[j]);
        }
      }
      const bool mustValid = minSure <= m2 * (1 - 16 * kU), mustInvalid = !(minMaybe <= m2 * (1 + 16 * kU));
      if ((!mustValid && !mustInvalid) || minMaybe * (1 + 16 * kU) < minSure) {
        ++skipped;
        continue;
      }
      const size_t o = b * N + s;
      const int32_t i = r.index[o];
      bool ok;
      if (mustInvalid) {
        ok = i == -1 && std::isinf(r.dist2[o]) && r.points[3 * o] == 0.f && r.points[3 * o + 1] == 0.f && r.points[3 * o + 2] == 0.f;
      } else {
        ok = i >= 0 && i < int32_t(M) && d[size_t(i)] <= (1 + 16 * kU) * minSure && std::fabs(double(r.dist2[o]) - d[size_t(i)]) <= 8 * kU * d[size_t(i)] &&
            r.points[3 * o] == t[3 * i] && r.points[3 * o + 1] == t[3 * i + 1] && r.points[3 * o + 2] == t[3 * i + 2];
      }
      bad += ok ? 0 : 1;
    }
  }
  std::printf("%s: %d wrong, %d undecided of %zu\n", what, bad, skipped, B * N);
  return bad + (size_t(skipped) * 100 > B * N ? 1 : 0);
}

int main() {
  std::vector<float> src, sn, tgt, tn;
  fill(src, sn, B * N, 0.37);
  fill(tgt, tn, B * M, 0.53);
  const std::vector<float> tgtShared(tgt.begin(), tgt.begin() + M * 3), tnShared(tn.begin(), tn.begin() + M * 3);
  int bad = 0;
  ClosestPointsOptions o;
  bad += verify("per element", findClosestPoints(B, src, tgt), src, tgt, false, nullptr, nullptr, o.maxDist, 0.f);
  o.maxDist = 0.25f;
  bad += verify("max_dist 0.25", findClosestPoints(B, src, tgt, o), src, tgt, false, nullptr, nullptr, o.maxDist, 0.f);
  o.minNormalDot = 0.2f;
  bad += verify("normals, max_dist 0.25", findClosestPoints(B, src, tgt, o, sn, tn), src, tgt, false, &sn, &tn, o.maxDist, o.minNormalDot);
  o.targetShared = true;
  o.maxDist = std::numeric_limits<float>::infinity();
  bad += verify("shared, normals", findClosestPoints(B, src, tgtShared, o, sn, tnShared), src, tgtShared, true, &sn, &tnShared, o.maxDist, o.minNormalDot);
  // a refusal becomes std::runtime_error
  int threw = 0;
  try {
    o.maxDist = -1.f;
    (void)findClosestPoints(B, src, tgtShared, o);
  } catch (const std::runtime_error&) {
    ++threw;
  }
  try {
    (void)findClosestPoints(B, src, tgt, {}, sn); // one of the two normal arrays
  } catch (const std::runtime_error&) {
    ++threw;
  }
  try {
    findClosestPoints(1, 1, 1, nullptr, nullptr, nullptr, nullptr, {}, nullptr, nullptr, nullptr, nullptr); // the device form, null pointers
  } catch (const std::runtime_error&) {
    ++threw;
  }
  if (threw != 3) {
    std::printf("FAIL: a refusal did not throw\n");
    return 1;
  }
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
