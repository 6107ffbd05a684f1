// GPU smoke test of the vertex normals in the C++ shell (include/momentum_amd/momentum_amd.hpp, DeviceMesh): three batch
// elements of a 13 x 5 torus grid (65 vertices, valence 6) plus two vertices of no triangle, against a double loop written
// here in double -- normals, sums and the position gradient of L = sum cotangent . normals.
//
// Bounds (u = 2^-24): the library rounds its double results once, so a normal is within 2u of the double value and a sum
// within 2u of the largest sum.  The backward pass is defined on the sums it is handed, so the loop here takes h_v from the
// float32 sums the library returned: the gradient is then a double result rounded once as well, held to 4u of the largest
// gradient entry of its batch element.
#include <cmath>
#include <cstdio>

#include "momentum_amd/momentum_amd.hpp"

using namespace momentum_amd;

constexpr size_t B = 3, NU = 13, NV = 5, V = NU * NV + 2, T = 2 * NU * NV;
constexpr double kU = 1.0 / 16777216.0, kPi = 3.14159265358979323846;

struct D3 {
  double x, y, z;
};
static D3 sub(D3 a, D3 b) {
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
static D3 add(D3 a, D3 b) {
  return {a.x + b.x, a.y + b.y, a.z + b.z};
}
static D3 cross(D3 a, D3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
static double dot(D3 a, D3 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
static D3 at(const std::vector<float>& a, size_t i) {
  return {double(a[3 * i]), double(a[3 * i + 1]), double(a[3 * i + 2])};
}

int main() {
  std::vector<int32_t> tri;
  auto id = [](size_t i, size_t j) { return int32_t((i % NU) * NV + (j % NV)); };
  for (size_t i = 0; i < NU; ++i) {
    for (size_t j = 0; j < NV; ++j) {
      tri.insert(tri.end(), {id(i, j), id(i + 1, j), id(i + 1, j + 1), id(i, j), id(i + 1, j + 1), id(i, j + 1)});
    }
  }
  std::vector<float> pos(B * V * 3), cot(B * V * 3);
  for (size_t b = 0; b < B; ++b) {
    for (size_t v = 0; v < V; ++v) {
      const double th = 2 * kPi * double(v / NV) / NU, ph = 2 * kPi * double(v % NV) / NV, ring = 0.3 + 0.1 * std::cos(ph);
      const double p[3] = {ring * std::cos(th), ring * std::sin(th), 0.1 * std::sin(ph)};
      for (size_t c = 0; c < 3; ++c) {
        const size_t i = (b * V + v) * 3 + c;
        pos[i] = float(p[c] + 0.004 * std::sin(1.7 * double(i) + 0.3) + 0.5 * double(b));
        cot[i] = float(std::cos(0.9 * double(i) + 1.0));
      }
    }
  }
  const DeviceMesh mesh(V, tri);
  if (mesh.numVertices() != V || mesh.numTriangles() != T || mmx_mesh_num_vertices(mesh.handle()) != int32_t(V) ||
      mmx_mesh_num_triangles(mesh.handle()) != int32_t(T)) {
    std::printf("FAIL: sizes\n");
    return 1;
  }
  const DeviceMesh::Normals got = mesh.vertexNormals(B, pos);
  const std::vector<float> grad = mesh.vertexNormalsBackward(B, pos, got.sums, cot);

  int bad = 0;
  for (size_t b = 0; b < B; ++b) {
    const size_t o = b * V;
    std::vector<D3> m(V, D3{0, 0, 0}), n(V, D3{0, 0, 0}), h(V, D3{0, 0, 0}), want(V, D3{0, 0, 0});
    for (size_t t = 0; t < T; ++t) {
      const size_t a = size_t(tri[3 * t]), bb = size_t(tri[3 * t + 1]), c = size_t(tri[3 * t + 2]);
      const D3 f = cross(sub(at(pos, o + bb), at(pos, o + a)), sub(at(pos, o + c), at(pos, o + a)));
      m[a] = add(m[a], f), m[bb] = add(m[bb], f), m[c] = add(m[c], f);
    }
    double mMax = 0, gMax = 0;
    for (size_t v = 0; v < V; ++v) {
      const double s = dot(m[v], m[v]);
      mMax = std::fmax(mMax, std::sqrt(s));
      if (s > 0) {
        const double len = std::sqrt(s);
        n[v] = {m[v].x / len, m[v].y / len, m[v].z / len};
      }
      const D3 ms = at(got.sums, o + v), g = at(cot, o + v); // (the sums the backward pass was given)
      const double ss = dot(ms, ms);
      if (ss > 0) {
        const double len = std::sqrt(ss), ng = dot(ms, g) / len;
        h[v] = {(g.x - ms.x / len * ng) / len, (g.y - ms.y / len * ng) / len, (g.z - ms.z / len * ng) / len};
      }
    }
    for (size_t t = 0; t < T; ++t) {
      const size_t k[3] = {size_t(tri[3 * t]), size_t(tri[3 * t + 1]), size_t(tri[3 * t + 2])};
      const D3 H = add(add(h[k[0]], h[k[1]]), h[k[2]]);
      for (size_t c = 0; c < 3; ++c) {
        want[k[c]] = add(want[k[c]], cross(sub(at(pos, o + k[(c + 1) % 3]), at(pos, o + k[(c + 2) % 3])), H));
      }
    }
    for (size_t v = 0; v < V; ++v) {
      gMax = std::fmax(gMax, std::fmax(std::fabs(want[v].x), std::fmax(std::fabs(want[v].y), std::fabs(want[v].z))));
    }
    for (size_t v = 0; v < V; ++v) {
      const D3 gn = at(got.normals, o + v), gm = at(got.sums, o + v), gg = at(grad, o + v);
      const bool isolated = v >= NU * NV;
      bool ok;
      if (isolated) {
        ok = gn.x == 0 && gn.y == 0 && gn.z == 0 && gm.x == 0 && gm.y == 0 && gm.z == 0 && gg.x == 0 && gg.y == 0 && gg.z == 0;
      } else {
        const D3 dn = sub(gn, n[v]), dm = sub(gm, m[v]), dg = sub(gg, want[v]);
        ok = std::sqrt(dot(dn, dn)) <= 2 * kU && std::sqrt(dot(dm, dm)) <= 2 * kU * mMax && std::sqrt(dot(dg, dg)) <= 4 * kU * gMax &&
            std::fabs(dot(gn, gn) - 1.0) <= 4 * kU;
      }
      if (!ok) {
        ++bad;
        std::printf("element %zu vertex %zu: normal %g %g %g want %g %g %g; gradient %g %g %g want %g %g %g\n", b, v, gn.x, gn.y, gn.z, n[v].x, n[v].y,
                    n[v].z, gg.x, gg.y, gg.z, want[v].x, want[v].y, want[v].z);
      }
    }
  }
  // a refusal becomes std::runtime_error
  int threw = 0;
  try {
    std::vector<int32_t> wrong = tri;
    wrong[5] = int32_t(V);
    const DeviceMesh m2(V, wrong);
  } catch (const std::runtime_error&) {
    ++threw;
  }
  try {
    (void)mesh.vertexNormals(B + 1, pos); // sizes that do not match
  } catch (const std::runtime_error&) {
    ++threw;
  }
  try {
    mesh.vertexNormals(1, nullptr, nullptr, nullptr, nullptr); // the device form, null pointers
  } catch (const std::runtime_error&) {
    ++threw;
  }
  try {
    mesh.vertexNormalsBackward(0, nullptr, nullptr, nullptr, nullptr, nullptr);
  } catch (const std::runtime_error&) {
    ++threw;
  }
  if (threw != 4) {
    std::printf("FAIL: a refusal did not throw\n");
    return 1;
  }
  if (bad != 0) {
    std::printf("FAIL: %d vertices\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
