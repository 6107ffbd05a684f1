// GPU smoke test of the vertex constraints' Gauss-Newton terms in the C++ shell (include/momentum_amd/momentum_amd.hpp,
// DeviceSkin::normalEquations over mmx_skin_normal_equations_host): on momentum's 3-joint test character with the five-vertex,
// K = 4 skin of the Python tests (tests/skinning_reference.py hand_skin) and a perturbed inverse bind, with one parameter
// disabled, H = J^T J, g = J^T r and the error equal what the forward kinematics and the skinning formula written here in
// double give, J by central differences (h = 1e-6) of the scaled rows.  Two calls: four plane constraints on triangle corners
// with barycentric weights (one of them skipped by a -1 index, one by a zero weight with a NaN target behind it), and position
// constraints on every vertex (vertex list empty).
//
// Bounds: the float32 run of the torch reference (tests/vertex_constraints_reference.py) deviates from its float64 run on these
// inputs by at most 2.42e-7 max|H|, 2.47e-7 max|g| and 1.05e-7 of the error (largest of the four elements and the two calls); the
// GPU is allowed max(4 x that, 16 x 2^-24 = 9.54e-7) against the double values, 9.7e-7 / 9.9e-7 / 9.6e-7 -- the rule of
// tests/test_gpu_vertex_normal_equations.py.  The central differences themselves are good to 1e-9.
#include <cmath>
#include <cstdio>
#include <limits>

#include "momentum_amd/momentum_amd.hpp"

using namespace momentum_amd;

static Character createTestCharacter(size_t n) {
  Character c;
  Joint j;
  j.name = "root";
  c.skeleton.joints.push_back(j);
  for (size_t i = 1; i < n; ++i) {
    j.name = "joint" + std::to_string(i);
    j.parent = i - 1;
    j.translationOffset = {0.f, 1.f, 0.f};
    c.skeleton.joints.push_back(j);
  }
  auto& pt = c.parameterTransform;
  pt.name = {"root_tx", "root_ty", "root_tz", "root_rx", "root_ry", "root_rz", "scale_global", "joint1_rx", "shared_rz"};
  const int rxStart = int(pt.name.size());
  for (size_t i = 2; i < n; ++i) {
    pt.name.push_back("joint" + std::to_string(i) + "_rx");
  }
  std::vector<ParameterTransform::Triplet> t;
  for (int d = 0; d < 7; ++d) {
    t.push_back({d, d, 1.f});
  }
  t.push_back({1 * 7 + 3, 7, 1.f});
  t.push_back({1 * 7 + 5, 8, 0.5f});
  t.push_back({2 * 7 + 5, 8, 0.5f});
  for (size_t i = 2; i < n; ++i) {
    t.push_back({int(i * 7 + 3), rxStart + int(i) - 2, 1.f});
  }
  pt.setFromTriplets(n, t);
  return c;
}

constexpr size_t B = 4, J = 3, P = 10, V = 5, K = 4, N = 9; // N: enabled parameters (parameter 4 is off)
static const int32_t kJoint[V * K] = {0, 1, 2, 2, 1, 0, 2, 0, 0, 2, 2, 2, 1, 1, 2, 0, 0, 1, 0, 1};
static const float kWeight[V * K] = {0.7f, 0.3f, 0.f, 0.f, 0.25f, 0.75f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.5f, 0.125f, 0.f, 0.375f, 0.4f, 0.3f, 0.2f, 0.1f};
static const float kRest[V * 3] = {0.1f, 0.2f, -0.3f, 0.3f, 1.1f, 0.2f, -0.2f, 0.4f, 0.1f, 0.05f, 1.6f, -0.1f, 0.2f, 0.9f, 0.3f};

struct Q {
  double x, y, z, w;
};
static Q mul(const Q& a, const Q& b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x,
          a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
static void rot(const Q& q, const double* v, double* o) {
  const double ux = 2 * (q.y * v[2] - q.z * v[1]), uy = 2 * (q.z * v[0] - q.x * v[2]), uz = 2 * (q.x * v[1] - q.y * v[0]);
  o[0] = v[0] + q.w * ux + (q.y * uz - q.z * uy);
  o[1] = v[1] + q.w * uy + (q.z * ux - q.x * uz);
  o[2] = v[2] + q.w * uz + (q.x * uy - q.y * ux);
}
// the 3-joint character's forward kinematics in double: theta [10] -> state [3][8]
static void forward(const double* th, double* st) {
  double jp[3][7] = {};
  for (int d = 0; d < 7; ++d) {
    jp[0][d] = th[d];
  }
  jp[1][3] = th[7], jp[1][5] = 0.5 * th[8], jp[2][5] = 0.5 * th[8], jp[2][3] = th[9];
  double tp[3] = {0, 0, 0}, sp = 1.0;
  Q qp{0, 0, 0, 1};
  for (int j = 0; j < 3; ++j) {
    const double* p = jp[j];
    const Q ql = mul(mul(Q{0, 0, std::sin(0.5 * p[5]), std::cos(0.5 * p[5])}, Q{0, std::sin(0.5 * p[4]), 0, std::cos(0.5 * p[4])}), Q{std::sin(0.5 * p[3]), 0, 0, std::cos(0.5 * p[3])});
    const double tl[3] = {sp * p[0], sp * ((j > 0 ? 1.0 : 0.0) + p[1]), sp * p[2]};
    double r[3];
    rot(qp, tl, r);
    for (int k = 0; k < 3; ++k) {
      tp[k] += r[k];
    }
    qp = mul(qp, ql);
    sp *= std::exp2(p[6]);
    double* o = st + 8 * j;
    o[0] = tp[0], o[1] = tp[1], o[2] = tp[2], o[3] = qp.x, o[4] = qp.y, o[5] = qp.z, o[6] = qp.w, o[7] = sp;
  }
}
// linear-blend skinning in double: state [J][8] -> vertices [V][3]
static void skin(const double* st, const float* inv, double* out) {
  for (size_t v = 0; v < V; ++v) {
    double acc[3] = {0, 0, 0};
    for (size_t k = 0; k < K; ++k) {
      const double w = double(kWeight[v * K + k]);
      if (w == 0.0) {
        continue;
      }
      const size_t j = size_t(kJoint[v * K + k]);
      const float* m = inv + 12 * j;
      double p[3], r[3];
      for (int i = 0; i < 3; ++i) {
        p[i] = double(m[4 * i]) * double(kRest[3 * v]) + double(m[4 * i + 1]) * double(kRest[3 * v + 1]) + double(m[4 * i + 2]) * double(kRest[3 * v + 2]) + double(m[4 * i + 3]);
      }
      const double* s = st + 8 * j;
      rot(Q{s[3], s[4], s[5], s[6]}, p, r);
      for (int i = 0; i < 3; ++i) {
        acc[i] += w * (s[i] + s[7] * r[i]);
      }
    }
    out[3 * v] = acc[0], out[3 * v + 1] = acc[1], out[3 * v + 2] = acc[2];
  }
}

// the scaled rows of one element in double; skipped constraints give zero rows
static std::vector<double> rows(const double* th, const float* inv, const VertexConstraints& c, size_t b, size_t count) {
  double st[J * 8], out[V * 3];
  forward(th, st);
  skin(st, inv, out);
  const bool plane = !c.normal.empty();
  std::vector<double> r(count * (plane ? 1 : 3), 0.0);
  for (size_t i = 0; i < count; ++i) {
    const size_t at = b * count + i;
    const float w = c.weight.empty() ? 1.f : c.weight[at];
    bool act = w > 0.f;
    for (size_t s = 0; s < c.corners && !c.vertex.empty(); ++s) {
      const int32_t v = c.vertex[at * c.corners + s];
      act = act && v >= 0 && v < int32_t(V);
    }
    if (!act) {
      continue;
    }
    double x[3] = {0, 0, 0};
    for (size_t s = 0; s < c.corners; ++s) {
      const size_t v = c.vertex.empty() ? i : size_t(c.vertex[at * c.corners + s]);
      const double beta = c.corners == 3 ? double(c.barycentric[at * 3 + s]) : 1.0;
      for (int k = 0; k < 3; ++k) {
        x[k] += beta * out[3 * v + k];
      }
    }
    const double sigma = std::sqrt(double(c.functionWeight) * double(w));
    if (plane) {
      for (int k = 0; k < 3; ++k) {
        r[i] += sigma * double(c.normal[at * 3 + k]) * (x[k] - double(c.target[at * 3 + k]));
      }
    } else {
      for (int k = 0; k < 3; ++k) {
        r[3 * i + k] = sigma * (x[k] - double(c.target[at * 3 + k]));
      }
    }
  }
  return r;
}

static int compare(const char* what, const DeviceSkin& skinDev, BatchedSkeletonSolverFunction& fn, const std::vector<float>& theta, const float* inv,
                   const VertexConstraints& c, size_t count) {
  const VertexNormalEquations ne = skinDev.normalEquations(fn, theta, c);
  if (ne.n != N || ne.jtj.size() != B * N * N || ne.jtr.size() != B * N || ne.error.size() != B) {
    std::printf("FAIL %s: sizes (n = %zu)\n", what, ne.n);
    return 1;
  }
  int bad = 0;
  for (size_t b = 0; b < B; ++b) {
    double th[P];
    for (size_t p = 0; p < P; ++p) {
      th[p] = double(theta[b * P + p]);
    }
    const std::vector<double> r = rows(th, inv, c, b, count);
    std::vector<std::vector<double>> cols; // d rows / d enabled parameter
    for (size_t p = 0; p < P; ++p) {
      if (p == 4) {
        continue;
      }
      const double h = 1e-6, keep = th[p];
      th[p] = keep + h;
      const std::vector<double> rp = rows(th, inv, c, b, count);
      th[p] = keep - h;
      const std::vector<double> rm = rows(th, inv, c, b, count);
      th[p] = keep;
      std::vector<double> col(r.size());
      for (size_t i = 0; i < r.size(); ++i) {
        col[i] = (rp[i] - rm[i]) / (2 * h);
      }
      cols.push_back(col);
    }
    double hmax = 0, hdiff = 0, gmax = 0, gdiff = 0, err = 0;
    bool symmetric = true;
    for (size_t i = 0; i < N; ++i) {
      double g = 0;
      for (size_t k = 0; k < r.size(); ++k) {
        g += cols[i][k] * r[k];
      }
      gmax = std::fmax(gmax, std::fabs(g));
      gdiff = std::fmax(gdiff, std::fabs(g - double(ne.jtr[b * N + i])));
      for (size_t j = 0; j < N; ++j) {
        double hij = 0;
        for (size_t k = 0; k < r.size(); ++k) {
          hij += cols[i][k] * cols[j][k];
        }
        hmax = std::fmax(hmax, std::fabs(hij));
        hdiff = std::fmax(hdiff, std::fabs(hij - double(ne.jtj[(b * N + i) * N + j])));
        symmetric = symmetric && ne.jtj[(b * N + i) * N + j] == ne.jtj[(b * N + j) * N + i];
      }
    }
    for (double x : r) {
      err += x * x;
    }
    const double ediff = std::fabs(err - ne.error[b]);
    const bool ok = hdiff <= 9.7e-7 * hmax && gdiff <= 9.9e-7 * gmax && ediff <= 9.6e-7 * err && hmax > 0.1 && gmax > 0.1 && err > 0.01 && symmetric;
    std::printf(
        "%s, element %zu: H off by %.3g of max|H| (bound 9.7e-7), g by %.3g of max|g| (bound 9.9e-7), the error by %.3g (bound 9.6e-7), H %s%s\n", what, b,
        hdiff / hmax, gdiff / gmax, ediff / err, symmetric ? "symmetric" : "NOT symmetric", ok ? "" : "  FAIL");
    bad += ok ? 0 : 1;
  }
  return bad;
}

int main() {
  const Character character = createTestCharacter(J);
  DeviceCharacter dev(character, 0);
  BatchedSkeletonSolverFunction fn(dev, B, {0}, {});
  if (fn.getNumParameters() != P || fn.numEnabledParameters() != P) {
    std::printf("FAIL: P = %zu\n", fn.getNumParameters());
    return 1;
  }
  ParameterSet enabled(P, true);
  enabled[4] = false;
  fn.setEnabledParameters(enabled);
  std::vector<float> inv(J * 12), theta(B * P);
  for (size_t j = 0; j < J; ++j) { // the rest pose's inverse (joint j sits at (0, j, 0)), every entry perturbed
    for (size_t i = 0; i < 12; ++i) {
      const double base = (i == 0 || i == 5 || i == 10) ? 1.0 : (i == 7 ? -double(j) : 0.0);
      inv[12 * j + i] = float(base + 0.1 * std::sin(double(i + 2 * j)));
    }
  }
  for (size_t b = 0; b < B; ++b) {
    for (size_t p = 0; p < P; ++p) {
      theta[b * P + p] = float(0.4 * std::sin(1.7 * double(p) + double(b)));
    }
  }
  const DeviceSkin skinDev(
      dev, K, std::vector<int32_t>(kJoint, kJoint + V * K), std::vector<float>(kWeight, kWeight + V * K), inv, std::vector<float>(kRest, kRest + V * 3));
  // ---- four plane constraints on triangle corners
  const size_t C = 4;
  static const int32_t kCorners[C * 3] = {0, 1, 2, 3, 4, 0, 1, 3, 4, 2, 4, 1};
  VertexConstraints tri;
  tri.corners = 3;
  tri.functionWeight = 0.7f;
  for (size_t b = 0; b < B; ++b) {
    for (size_t i = 0; i < C; ++i) {
      double w[3] = {1.0 + 0.5 * std::sin(double(b + i)), 1.0 + 0.5 * std::cos(double(2 * b + i)), 1.0 + 0.5 * std::sin(double(b + 3 * i) + 1.0)};
      const double sum = w[0] + w[1] + w[2];
      for (int k = 0; k < 3; ++k) {
        tri.vertex.push_back(kCorners[3 * i + size_t(k)]);
        tri.barycentric.push_back(float(w[k] / sum));
        tri.target.push_back(float(0.5 * std::sin(1.1 * double(3 * i + size_t(k)) + 0.7 * double(b))));
        tri.normal.push_back(float(std::cos(0.8 * double(3 * i + size_t(k)) + 0.3 * double(b))));
      }
      tri.weight.push_back(float(1.0 + 0.5 * std::sin(double(i) + 0.4 * double(b))));
    }
  }
  tri.vertex[(1 * C + 2) * 3 + 1] = -1; // element 1, constraint 2: no triangle found
  tri.weight[2 * C + 0] = 0.f; // element 2, constraint 0: weight 0 ...
  tri.target[(2 * C + 0) * 3 + 1] = std::numeric_limits<float>::quiet_NaN(); // ... with a NaN behind it
  int bad = compare("plane, corners = 3", skinDev, fn, theta, inv.data(), tri, C);
  // ---- position constraints on every vertex
  VertexConstraints all;
  for (size_t b = 0; b < B; ++b) {
    for (size_t i = 0; i < V * 3; ++i) {
      all.target.push_back(float(0.5 * std::cos(0.9 * double(i) + 0.5 * double(b))));
    }
  }
  bad += compare("position, every vertex", skinDev, fn, theta, inv.data(), all, V);
  // a refusal becomes std::runtime_error
  bool threw = false;
  try {
    VertexConstraints wrong = tri;
    wrong.corners = 2;
    wrong.vertex.resize(B * C * 2);
    (void)skinDev.normalEquations(fn, theta, wrong);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  if (!threw) {
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
