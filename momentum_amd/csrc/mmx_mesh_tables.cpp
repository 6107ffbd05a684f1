// mmx_mesh_tables.cpp -- the vertex-sorted incidence list of a triangle mesh and its per-wave layout (mmx_mesh_tables.hpp).
#include "mmx_mesh_tables.hpp"

#include <algorithm>

namespace mmx {

int32_t validateMesh(int32_t V, int32_t T, const int32_t* triangles, std::string& err) {
  auto bad = [&](const char* what) {
    err = what;
    return int32_t(MMX_ERR_INVALID_ARGUMENT);
  };
  if (V < 1 || T < 1) {
    return bad("num_vertices and num_triangles must be >= 1");
  }
  if (triangles == nullptr) {
    return bad("triangles is null");
  }
  if (int64_t(T) * 3 > int64_t(INT32_MAX)) {
    return bad("3 * num_triangles exceeds 2^31 - 1");
  }
  for (size_t i = 0; i < size_t(T) * 3; ++i) {
    if (triangles[i] < 0 || triangles[i] >= V) {
      return bad("vertex index out of range");
    }
  }
  return MMX_OK;
}

const char* meshBatchRefusal(int32_t V, int32_t batch, int64_t* workgroups) {
  if (batch < 1) {
    return "batch must be >= 1";
  }
  if (int64_t(batch) * int64_t(V) > int64_t(INT32_MAX) / 3) { // (the product of two int32 fits int64; three times it may not)
    return "batch * num_vertices * 3 exceeds 2^31 - 1";
  }
  const int64_t n = int64_t(batch) * ((int64_t(V) + kMeshThreads - 1) / kMeshThreads);
  if (n > int64_t(INT32_MAX)) {
    return "the launch grid exceeds 2^31 - 1 workgroups";
  }
  if (workgroups != nullptr) {
    *workgroups = n;
  }
  return nullptr;
}

MeshTables buildMeshTables(int32_t V, int32_t T, const int32_t* tri, bool layout) {
  MeshTables t;
  // counting sort by vertex; triangles and corners are visited in ascending order, so each vertex's entries come out sorted
  t.vertexStart.assign(size_t(V) + 1, 0);
  const size_t E = size_t(T) * 3;
  for (size_t i = 0; i < E; ++i) {
    ++t.vertexStart[size_t(tri[i]) + 1];
  }
  for (int32_t v = 0; v < V; ++v) {
    t.maxValence = std::max(t.maxValence, t.vertexStart[size_t(v) + 1]);
    t.vertexStart[size_t(v) + 1] += t.vertexStart[size_t(v)];
  }
  t.entryTriangle.resize(E), t.entryCorner.resize(E);
  std::vector<int32_t> next(t.vertexStart.begin(), t.vertexStart.end() - 1);
  for (size_t i = 0; i < E; ++i) {
    const size_t e = size_t(next[size_t(tri[i])]++);
    t.entryTriangle[e] = int32_t(i / 3), t.entryCorner[e] = int32_t(i % 3);
  }
  if (!layout) {
    return t;
  }
  // the device layout: per group of 64 vertices, rows of 64 records
  const int32_t G = (V + kMeshGroup - 1) / kMeshGroup;
  t.groupBase.resize(size_t(G)), t.groupMax.resize(size_t(G));
  int64_t total = 0;
  for (int32_t g = 0; g < G; ++g) {
    int32_t rows = 0;
    for (int32_t v = g * kMeshGroup; v < std::min(V, (g + 1) * kMeshGroup); ++v) {
      rows = std::max(rows, t.vertexStart[size_t(v) + 1] - t.vertexStart[size_t(v)]);
    }
    t.groupMax[size_t(g)] = rows;
    t.groupBase[size_t(g)] = int32_t(std::min<int64_t>(total, INT32_MAX));
    total += int64_t(rows) * kMeshGroup;
  }
  if (total > int64_t(INT32_MAX)) {
    t.fits = false;
    return t;
  }
  t.records.assign(size_t(total) * 4, 0);
  for (int32_t g = 0; g < G; ++g) {
    for (int32_t lane = 0; lane < kMeshGroup; ++lane) {
      const int32_t v = g * kMeshGroup + lane;
      const int32_t e0 = v < V ? t.vertexStart[size_t(v)] : 0, count = v < V ? t.vertexStart[size_t(v) + 1] - e0 : 0;
      for (int32_t i = 0; i < t.groupMax[size_t(g)]; ++i) {
        int32_t* r = t.records.data() + (size_t(t.groupBase[size_t(g)]) + size_t(i) * kMeshGroup + size_t(lane)) * 4;
        if (i < count) {
          const int32_t* abc = tri + size_t(t.entryTriangle[size_t(e0 + i)]) * 3;
          r[0] = abc[0], r[1] = abc[1], r[2] = abc[2], r[3] = t.entryCorner[size_t(e0 + i)];
        } else {
          r[3] = -1;
        }
      }
    }
  }
  return t;
}

} // namespace mmx
