// The tables of the vertex-normal kernels (buildMeshTables, momentum_amd/csrc/mmx_mesh_tables.hpp) against restatements
// written here: the vertex-sorted incidence list against a std::stable_sort by vertex of the (triangle, corner) pairs taken in
// order, and the per-wave layout -- walking the rows of a vertex's group at its lane gives exactly that vertex's entries, in
// order, as (a, b, c, corner) of the entry's triangle, then padding (corner -1, indices 0) to the group's longest list; groups
// follow each other without gap or overlap; lanes past V are padding.  Also validateMesh and meshBatchRefusal at their
// edges.  Stand-alone: links mmx_mesh_tables.cpp only, needs no GPU (tests/test_mesh_tables_host.py builds it with the
// address and undefined-behaviour sanitizers).
#include "../../momentum_amd/csrc/mmx_mesh_tables.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

namespace {

using Ints = std::vector<int32_t>;

const char* g_case = "";
#define CHECK(...)                                                                     \
  do {                                                                                 \
    if (!(__VA_ARGS__)) {                                                              \
      std::printf("FAILED [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #__VA_ARGS__); \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

mmx::MeshTables checkMesh(const char* name, int32_t V, const Ints& tri) {
  g_case = name;
  const int32_t T = int32_t(tri.size() / 3);
  std::string err;
  CHECK(mmx::validateMesh(V, T, tri.data(), err) == MMX_OK);
  const mmx::MeshTables t = mmx::buildMeshTables(V, T, tri.data(), true);
  // ---- the incidence list
  Ints pairs(tri.size());
  for (size_t i = 0; i < pairs.size(); ++i) {
    pairs[i] = int32_t(i);
  }
  std::stable_sort(pairs.begin(), pairs.end(), [&](int32_t a, int32_t b) { return tri[size_t(a)] < tri[size_t(b)]; });
  CHECK(t.entryTriangle.size() == pairs.size() && t.entryCorner.size() == pairs.size());
  CHECK(int32_t(t.vertexStart.size()) == V + 1 && t.vertexStart[0] == 0 && size_t(t.vertexStart[size_t(V)]) == pairs.size());
  int32_t longest = 0;
  for (size_t e = 0; e < pairs.size(); ++e) {
    CHECK(t.entryTriangle[e] == pairs[e] / 3 && t.entryCorner[e] == pairs[e] % 3);
    const int32_t v = tri[size_t(pairs[e])];
    CHECK(int32_t(e) >= t.vertexStart[size_t(v)] && int32_t(e) < t.vertexStart[size_t(v) + 1]);
  }
  for (int32_t v = 0; v < V; ++v) {
    CHECK(t.vertexStart[size_t(v)] <= t.vertexStart[size_t(v) + 1]);
    longest = std::max(longest, t.vertexStart[size_t(v) + 1] - t.vertexStart[size_t(v)]);
  }
  CHECK(t.maxValence == longest);
  // ---- the layout
  const int32_t G = (V + mmx::kMeshGroup - 1) / mmx::kMeshGroup;
  CHECK(t.fits && int32_t(t.groupBase.size()) == G && int32_t(t.groupMax.size()) == G);
  int64_t next = 0;
  for (int32_t g = 0; g < G; ++g) {
    CHECK(t.groupBase[size_t(g)] == next);
    int32_t rows = 0;
    for (int32_t lane = 0; lane < mmx::kMeshGroup; ++lane) {
      const int32_t v = g * mmx::kMeshGroup + lane;
      const int32_t e0 = v < V ? t.vertexStart[size_t(v)] : 0, count = v < V ? t.vertexStart[size_t(v) + 1] - e0 : 0;
      rows = std::max(rows, count);
      for (int32_t i = 0; i < t.groupMax[size_t(g)]; ++i) {
        const size_t r = (size_t(next) + size_t(i) * mmx::kMeshGroup + size_t(lane)) * 4;
        CHECK(r + 3 < t.records.size());
        if (i < count) {
          const int32_t tr = t.entryTriangle[size_t(e0 + i)], c = t.entryCorner[size_t(e0 + i)];
          CHECK(t.records[r] == tri[size_t(tr) * 3] && t.records[r + 1] == tri[size_t(tr) * 3 + 1] && t.records[r + 2] == tri[size_t(tr) * 3 + 2]);
          CHECK(t.records[r + 3] == c && t.records[r + size_t(c)] == v);
        } else {
          CHECK(t.records[r] == 0 && t.records[r + 1] == 0 && t.records[r + 2] == 0 && t.records[r + 3] == -1);
        }
      }
    }
    CHECK(t.groupMax[size_t(g)] == rows); // no row that every lane pads
    next += int64_t(rows) * mmx::kMeshGroup;
  }
  CHECK(size_t(next) * 4 == t.records.size());
  return t;
}

Ints randomMesh(int32_t V, int32_t T, unsigned seed, int32_t lowest = 0) {
  std::mt19937 rng(seed);
  std::uniform_int_distribution<int32_t> any(lowest, V - 1);
  Ints tri(size_t(T) * 3);
  for (int32_t& x : tri) {
    x = any(rng); // (repeated corners happen)
  }
  return tri;
}

} // namespace

int main() {
  // ---- seeded random meshes around the group and workgroup sizes
  unsigned seed = 1;
  for (int32_t V : {1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000}) {
    for (int32_t T : {1, 2, 7, 300, 2500}) {
      char name[64];
      std::snprintf(name, sizeof name, "random V=%d T=%d", V, T);
      checkMesh(name, V, randomMesh(V, T, seed++));
    }
  }
  // ---- whole groups of isolated vertices: groups without rows
  {
    const mmx::MeshTables t = checkMesh("isolated groups", 300, randomMesh(300, 40, 77, 200));
    CHECK(t.groupMax[0] == 0 && t.groupMax[1] == 0 && t.groupMax[2] == 0 && t.groupBase[3] == 0);
  }
  // ---- a fan: hub 0 of valence 1000; its group runs 1000 rows, the others 2
  {
    Ints tri;
    for (int32_t i = 0; i < 1000; ++i) {
      tri.insert(tri.end(), {0, 1 + i, 1 + (i + 1) % 1000});
    }
    const mmx::MeshTables t = checkMesh("fan", 1001, tri);
    CHECK(t.maxValence == 1000 && t.groupMax[0] == 1000 && t.groupMax[1] == 2 && t.groupMax.back() == 2);
  }
  // ---- a vertex at two and at three corners of one triangle
  {
    const mmx::MeshTables t = checkMesh("repeated corners", 3, {1, 1, 2, 0, 0, 0});
    CHECK(t.vertexStart == Ints({0, 3, 5, 6}) && t.entryCorner == Ints({0, 1, 2, 0, 1, 2}));
  }
  // ---- one triangle
  {
    const mmx::MeshTables t = checkMesh("one triangle", 3, {2, 0, 1});
    CHECK(t.groupMax == Ints({1}) && t.records.size() == 64 * 4);
    CHECK(Ints(t.records.begin(), t.records.begin() + 16) == Ints({2, 0, 1, 1, 2, 0, 1, 2, 2, 0, 1, 0, 0, 0, 0, -1}));
  }
  // ---- validateMesh and meshBatchRefusal
  g_case = "refusals";
  {
    std::string err;
    const Ints tri{0, 1, 2};
    CHECK(mmx::validateMesh(3, 1, tri.data(), err) == MMX_OK);
    CHECK(mmx::validateMesh(0, 1, tri.data(), err) == MMX_ERR_INVALID_ARGUMENT);
    CHECK(mmx::validateMesh(3, 0, tri.data(), err) == MMX_ERR_INVALID_ARGUMENT);
    CHECK(mmx::validateMesh(3, 1, nullptr, err) == MMX_ERR_INVALID_ARGUMENT);
    CHECK(mmx::validateMesh(2, 1, tri.data(), err) == MMX_ERR_INVALID_ARGUMENT && err.find("out of range") != std::string::npos);
    CHECK(mmx::validateMesh(3, 715827883, tri.data(), err) == MMX_ERR_INVALID_ARGUMENT && err.find("2^31") != std::string::npos); // 3 T = 2^31 + 1
    int64_t n = -1;
    CHECK(mmx::meshBatchRefusal(257, 3, &n) == nullptr && n == 6);
    CHECK(mmx::meshBatchRefusal(256, 1, &n) == nullptr && n == 1);
    CHECK(mmx::meshBatchRefusal(256, 0, &n) != nullptr && mmx::meshBatchRefusal(256, -2, &n) != nullptr && n == 1);
    CHECK(mmx::meshBatchRefusal(1, 715827882, &n) == nullptr && n == 715827882); // B V 3 = 2^31 - 2
    CHECK(mmx::meshBatchRefusal(1, 715827883, &n) != nullptr && n == 715827882); // 2^31 + 1
    CHECK(mmx::meshBatchRefusal(2147483647, 2147483647, &n) != nullptr);
  }
  std::printf("OK\n");
  return 0;
}
