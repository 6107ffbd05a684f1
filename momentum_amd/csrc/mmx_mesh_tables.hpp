// mmx_mesh_tables.hpp -- host-side bookkeeping of the vertex normals of a triangle mesh (mmx_vertex_normals /
// mmx_vertex_normals_backward): no HIP here, so it is checked bit-exactly on the CPU (tests/test_mesh_tables_host.py through
// mmx_host_mesh_tables, tests/cpp/test_mesh_tables.cpp).
//
// Both kernels are gathers, one lane per vertex, and their summation order is fixed by ONE table, the vertex-sorted incidence
// list: every (triangle, corner) pair sorted by (vertex, triangle, corner), with vertexStart [V + 1] as the index.  A vertex
// that sits at two corners of one triangle has two entries; a vertex of no triangle has none.
//
// What the kernels read is that list transposed per group of 64 vertices (one wavefront): group g owns groupMax[g] rows of 64
// records, record (i, lane) = entry i of vertex 64 g + lane, so that a wave's loads of "entry i of my vertex" are contiguous.
// A record is four int32: the triangle's three indices in the triangle's own corner order and the corner this vertex sits at
// (-1: padding, the vertex has fewer than i + 1 entries or lies past V; its three indices are 0, a valid vertex).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmx.h"

namespace mmx {
#pragma GCC visibility push(hidden)

constexpr int32_t kMeshGroup = 64; // vertices per group = lanes of a wavefront
constexpr int32_t kMeshThreads = 256; // vertices per workgroup of either kernel

// Every check of a mesh that needs no device: V >= 1, T >= 1, triangles not null, 3 T <= 2^31 - 1, every index in [0, V).
// MMX_OK or MMX_ERR_INVALID_ARGUMENT with `err` set (without the function's name).
int32_t validateMesh(int32_t V, int32_t T, const int32_t* triangles, std::string& err);
// null, or why a batch of B instances of V vertices cannot be launched: batch < 1, B V 3 beyond 2^31 - 1, or a grid beyond
// 2^31 - 1 workgroups.  *workgroups = B ceil(V / kMeshThreads), an instance's workgroups adjacent.
const char* meshBatchRefusal(int32_t V, int32_t batch, int64_t* workgroups);

struct MeshTables {
  std::vector<int32_t> vertexStart; // [V + 1]
  std::vector<int32_t> entryTriangle, entryCorner; // [3 T] sorted by (vertex, triangle, corner)
  int32_t maxValence = 0; // the longest entry list
  // the device layout
  std::vector<int32_t> groupBase, groupMax; // [numGroups]: first record (in records) and rows of group g
  std::vector<int32_t> records; // [numRecords][4] = (a, b, c, corner)
  bool fits = true; // false: the padded layout exceeds 2^31 - 1 records (records is then empty)
};
// (the mesh must have passed validateMesh); `layout` false skips the device layout
MeshTables buildMeshTables(int32_t V, int32_t T, const int32_t* triangles, bool layout);

#pragma GCC visibility pop
} // namespace mmx
