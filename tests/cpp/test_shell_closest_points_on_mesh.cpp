// GPU smoke test of the closest-point-on-mesh query in the C++ shell (include/momentum_amd/momentum_amd.hpp,
// DeviceMesh::closestPoints / findClosestPointsOnMesh over mmx_closest_points_on_mesh_host): three batch elements of 70 sources
// against an 8 x 6 grid of 96 triangles over a wavy height field (per element, then shared, then with a finite max_dist),
// against a brute force written here in double.
//
// The double yardstick minimises |p - a - s e1 - t e2|^2 over the triangle by trying the interior solution and the three edge
// segments.  Bounds (u = 2^-24, R = the largest distance from the source to a corner, K = 64 as in
// tests/closest_points_on_mesh_reference.py): the returned face's double distance is within K u 2R of the smallest one,
// sqrt(dist2) within K u R of the returned face's, the weights are >= 0 and sum to 1 within 4u, their point in double is within
// K u R of optimal and `points` within 4u of that point's scale; a source is skipped where the double minimum sits within
// K u R of max_dist (the program counts them and fails above 1 %).
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "momentum_amd/momentum_amd.hpp"

using namespace momentum_amd;

constexpr size_t B = 3, N = 70, GX = 8, GY = 6, V = (GX + 1) * (GY + 1), T = 2 * GX * GY;
constexpr double kU = 1.0 / 16777216.0, kK = 64.0;

struct D3 {
  double x, y, z;
};
static D3 sub(D3 a, D3 b) {
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
static double dot(D3 a, D3 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
static D3 at(const float* p) {
  return {double(p[0]), double(p[1]), double(p[2])};
}
static double segment(D3 p, D3 a, D3 b) { // squared distance to the segment a-b
  const D3 e = sub(b, a);
  const double t = std::clamp(dot(sub(p, a), e) / dot(e, e), 0.0, 1.0);
  const D3 r = sub(sub(p, a), D3{t * e.x, t * e.y, t * e.z});
  return dot(r, r);
}
static double triangleDistance(D3 p, D3 a, D3 b, D3 c) {
  const D3 e1 = sub(b, a), e2 = sub(c, a), v = sub(p, a);
  const double d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), d1 = dot(e1, v), d2 = dot(e2, v);
  const double det = d11 * d22 - d12 * d12, s = (d22 * d1 - d12 * d2) / det, t = (d11 * d2 - d12 * d1) / det;
  double best = std::min({segment(p, a, b), segment(p, b, c), segment(p, c, a)});
  if (s >= 0 && t >= 0 && s + t <= 1) {
    const D3 r = sub(v, D3{s * e1.x + t * e2.x, s * e1.y + t * e2.y, s * e1.z + t * e2.z});
    best = std::min(best, dot(r, r));
  }
  return std::sqrt(best);
}

static int verify(
    const char* what, const ClosestPointsOnMesh& r, const std::vector<float>& src, const std::vector<float>& vtx, bool shared,
    const std::vector<int32_t>& tri, float maxDist) {
  int bad = 0, skipped = 0;
  for (size_t b = 0; b < B; ++b) {
    const float* vb = vtx.data() + (shared ? 0 : b * V * 3);
    for (size_t s = 0; s < N; ++s) {
      const size_t o = b * N + s;
      const D3 p = at(src.data() + o * 3);
      std::vector<double> d(T), R(T);
      size_t g = 0;
      for (size_t f = 0; f < T; ++f) {
        const D3 a = at(vb + 3 * tri[3 * f]), bb = at(vb + 3 * tri[3 * f + 1]), c = at(vb + 3 * tri[3 * f + 2]);
        d[f] = triangleDistance(p, a, bb, c);
        R[f] = std::sqrt(std::max({dot(sub(p, a), sub(p, a)), dot(sub(p, bb), sub(p, bb)), dot(sub(p, c), sub(p, c))}));
        g = d[f] < d[g] ? f : g;
      }
      const bool mustValid = d[g] <= double(maxDist) - kK * kU * R[g], mustInvalid = !(d[g] <= double(maxDist) + kK * kU * R[g]);
      if (!mustValid && !mustInvalid) {
        ++skipped;
        continue;
      }
      const int32_t f = r.faceIndex[o];
      const float* w = r.barycentric.data() + 3 * o;
      const float* q = r.points.data() + 3 * o;
      bool ok;
      if (mustInvalid) {
        ok = f == -1 && std::isinf(r.dist2[o]) && w[0] == 0.f && w[1] == 0.f && w[2] == 0.f && q[0] == 0.f && q[1] == 0.f && q[2] == 0.f;
      } else {
        ok = f >= 0 && f < int32_t(T);
        if (ok) {
          const D3 a = at(vb + 3 * tri[3 * f]), bb = at(vb + 3 * tri[3 * f + 1]), c = at(vb + 3 * tri[3 * f + 2]);
          const D3 x{w[0] * a.x + w[1] * bb.x + w[2] * c.x, w[0] * a.y + w[1] * bb.y + w[2] * c.y, w[0] * a.z + w[1] * bb.z + w[2] * c.z};
          const double scale = std::sqrt(std::max({dot(a, a), dot(bb, bb), dot(c, c)}));
          ok = d[f] <= d[g] + kK * kU * (R[f] + R[g]) && std::fabs(std::sqrt(double(r.dist2[o])) - d[f]) <= kK * kU * R[f] && w[0] >= 0.f && w[1] >= 0.f &&
              w[2] >= 0.f && std::fabs(double(w[0]) + double(w[1]) + double(w[2]) - 1.0) <= 4 * kU &&
              std::fabs(std::sqrt(dot(sub(x, p), sub(x, p))) - d[f]) <= kK * kU * R[f] && std::fabs(q[0] - x.x) <= 4 * kU * scale &&
              std::fabs(q[1] - x.y) <= 4 * kU * scale && std::fabs(q[2] - x.z) <= 4 * kU * scale;
        }
      }
      bad += ok ? 0 : 1;
    }
  }
  std::printf("%s: %d wrong, %d undecided of %zu\n", what, bad, skipped, B * N);
  return bad + (size_t(skipped) * 100 > B * N ? 1 : 0);
}

int main() {
  std::vector<float> vtx(B * V * 3), src(B * N * 3);
  std::vector<int32_t> tri;
  for (size_t b = 0; b < B; ++b) {
    for (size_t i = 0; i <= GX; ++i) {
      for (size_t j = 0; j <= GY; ++j) {
        float* p = vtx.data() + ((b * V) + i * (GY + 1) + j) * 3;
        p[0] = float(0.1 * double(i) + 0.01 * std::sin(3.0 * double(j) + double(b)));
        p[1] = float(0.1 * double(j) + 0.01 * std::cos(2.0 * double(i) + double(b)));
        p[2] = float(0.05 * std::sin(0.9 * double(i) + 0.3 * double(b)) * std::cos(0.7 * double(j)));
      }
    }
    for (size_t s = 0; s < N; ++s) {
      float* p = src.data() + (b * N + s) * 3;
      p[0] = float(0.4 + 0.5 * std::sin(0.37 * double(3 * s) + 0.3 + double(b)));
      p[1] = float(0.3 + 0.4 * std::sin(0.37 * double(3 * s + 1) + 0.3));
      p[2] = float((s % 3 == 0 ? 0.001 : 0.08) * std::sin(0.37 * double(3 * s + 2)));
    }
  }
  for (size_t i = 0; i < GX; ++i) {
    for (size_t j = 0; j < GY; ++j) {
      const int32_t v00 = int32_t(i * (GY + 1) + j), v10 = int32_t((i + 1) * (GY + 1) + j), v11 = v10 + 1, v01 = v00 + 1;
      tri.insert(tri.end(), {v00, v10, v11, v00, v11, v01});
    }
  }
  const std::vector<float> vtxShared(vtx.begin(), vtx.begin() + V * 3);
  DeviceMesh mesh(V, tri);
  int bad = 0;
  ClosestPointsOnMeshOptions o;
  bad += verify("per element", mesh.closestPoints(B, src, vtx), src, vtx, false, tri, o.maxDist);
  o.maxDist = 0.03f;
  bad += verify("max_dist 0.03", findClosestPointsOnMesh(mesh, B, src, vtx, o), src, vtx, false, tri, o.maxDist);
  o.verticesShared = true;
  bad += verify("shared, max_dist 0.03", findClosestPointsOnMesh(mesh, B, src, vtxShared, o), src, vtxShared, true, tri, o.maxDist);
  // a refusal becomes std::runtime_error
  int threw = 0;
  try {
    o.maxDist = -1.f;
    (void)mesh.closestPoints(B, src, vtxShared, o);
  } catch (const std::runtime_error&) {
    ++threw;
  }
  try {
    (void)mesh.closestPoints(B, src, vtxShared); // vertices of the wrong size
  } catch (const std::runtime_error&) {
    ++threw;
  }
  try {
    mesh.closestPoints(1, 1, nullptr, nullptr, {}, nullptr, nullptr, nullptr, nullptr, nullptr); // the device form, null pointers
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
