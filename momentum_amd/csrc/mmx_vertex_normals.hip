// mmx_vertex_normals.hip -- area-weighted vertex normals of a batch of posed triangle meshes, forward and backward (gfx950 /
// CDNA4, wave64; include/mmx.h: mmx_vertex_normals).  The counterpart of pymomentum.geometry.compute_vertex_normals and
// momentum's Mesh::updateNormals.  The mesh handle, both kernels, their launchers and the C-ABI entry points live here; the
// bookkeeping is mmx_mesh_tables.cpp.
//
//   c_t = (p_b - p_a) x (p_c - p_a)        m_v = sum of c_t over the entries of v        n_v = m_v / |m_v|
//
// Both kernels are GATHERS: a lane owns one vertex and walks that vertex's entries of the vertex-sorted incidence list in
// ascending (triangle, corner) order, so a sum's order is the list's and nothing is scattered -- no atomics, no scratch
// buffer, no second kernel.  The price is that a face vector is recomputed at each of the triangle's three vertices; it goes
// through ONE function (faceVector, no contraction left to the compiler, in the triangle's own corner order), so the three
// copies have the same bits.
// A 256-thread workgroup takes 256 consecutive vertices of one instance; an instance's workgroups are adjacent in the grid, so
// that its positions (12 V bytes) stay in L2 while its vertices gather them.  The list is read transposed per wavefront
// (mmx_mesh_tables.hpp): record (i, lane) of the wave's group is 16 bytes, the triangle's three indices and the corner, and a
// wave's loads of row i are 1 KB contiguous.  The wave runs as many rows as its longest list; a lane past its own list reads a
// padding record and adds nothing (a select, not a product: what padding points at may be NaN).
//
// vertexNormalsKernel          per entry three 12-byte position gathers; differences, cross product and sums in double; then
//     s = |m|^2, n = m / sqrt(s) (exact zeros for s == 0, NaN for a non-finite s), rounded once; streaming stores of n and,
//     where asked for, of m (float32: what the backward pass reads).
// vertexNormalsBackwardKernel  with h_v = (g_v - n_v (n_v . g_v)) / |m_v| = (s g_v - m_v (m_v . g_v)) / (s sqrt(s)) from the
//     stored sums and H_t = (h_a + h_b) + h_c:   dL/dp_x = sum over the entries (t, corner of x) of (p_next - p_prev) x H_t.
//     Per entry two position gathers, three sums and three cotangents.  h goes through ONE function (hOf), so H_t has the same
//     bits at each of the triangle's vertices.
// A vertex of very high valence (the hub of a fan) is walked by one lane while the other 63 of its wave idle: correct, slow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <string>

#include "../../include/mmx.h"
#include "mmx_mesh_tables.hpp"

namespace mmx {
int32_t failWith(int32_t code, const std::string& msg); // mmx_capi.hip: sets mmx_last_error()

namespace {

struct MeshDev {
  int32_t V, tiles /* workgroups per instance */, numGroups;
  const int4* records; // [numRecords] (a, b, c, corner)
  const int32_t* groupBase; // [numGroups]
  const int32_t* groupMax; // [numGroups]
};

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 load3(const float* p) {
  return V3{double(p[0]), double(p[1]), double(p[2])};
}
// Both products rounded, then the difference, wherever it is inlined -- never contracted into an fma: u x u is then three
// exact zeros (the two products of a component are the same number), so a triangle with a repeated vertex contributes zeros in
// any corner order; an fma would leave the rounding error of one product there.
__device__ __forceinline__ V3 cross(const V3& u, const V3& v) {
#pragma clang fp contract(off)
  return V3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
// THE face vector: every copy of a triangle's goes through this sequence and no other
__device__ __forceinline__ V3 faceVector(const V3& a, const V3& b, const V3& c) {
  return cross(V3{b.x - a.x, b.y - a.y, b.z - a.z}, V3{c.x - a.x, c.y - a.y, c.z - a.z});
}
__device__ __forceinline__ double norm2(const V3& m) {
  return fma(m.z, m.z, fma(m.y, m.y, m.x * m.x));
}
// THE cotangent of a vertex sum: h = (s g - m (m . g)) / (s sqrt(s)); zero for s == 0, NaN for a non-finite s
__device__ __forceinline__ V3 hOf(const float* sums, const float* grad) {
  const V3 m = load3(sums), g = load3(grad);
  const double s = norm2(m);
  const double mg = fma(m.z, g.z, fma(m.y, g.y, m.x * g.x));
  const double r = 1.0 / (s * sqrt(s));
  V3 h{fma(s, g.x, -(m.x * mg)) * r, fma(s, g.y, -(m.y * mg)) * r, fma(s, g.z, -(m.z * mg)) * r};
  const double kNaN = __builtin_nan("");
  if (s == 0.0) {
    h = V3{0.0, 0.0, 0.0};
  } else if (!(fabs(s) <= 1.79769313486231570815e308)) {
    h = V3{kNaN, kNaN, kNaN};
  }
  return h;
}

__device__ __forceinline__ void store3(float* o, float x, float y, float z) {
  __builtin_nontemporal_store(x, o);
  __builtin_nontemporal_store(y, o + 1);
  __builtin_nontemporal_store(z, o + 2);
}

__global__ void __launch_bounds__(kMeshThreads) vertexNormalsKernel(
    MeshDev mesh,
    const float* __restrict__ positions, // [B][V][3]
    float* __restrict__ normals, // [B][V][3] every entry written
    float* __restrict__ sums) { // null or [B][V][3] every entry written
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int b = int(blockIdx.x) / mesh.tiles, tile = int(blockIdx.x) % mesh.tiles;
  const int group = tile * (kMeshThreads / kMeshGroup) + wave;
  if (group >= mesh.numGroups) {
    return;
  }
  const int V = mesh.V, v = group * kMeshGroup + lane;
  const float* p = positions + size_t(b) * size_t(V) * 3;
  const int4* rec = mesh.records + size_t(mesh.groupBase[group]) + size_t(lane);
  const int rows = mesh.groupMax[group];
  double mx = 0.0, my = 0.0, mz = 0.0;
#pragma unroll 2
  for (int i = 0; i < rows; ++i) {
    const int4 r = rec[size_t(i) * kMeshGroup];
    const V3 a = load3(p + size_t(r.x) * 3), bb = load3(p + size_t(r.y) * 3), c = load3(p + size_t(r.z) * 3);
    const V3 f = faceVector(a, bb, c);
    const bool on = r.w >= 0;
    mx += on ? f.x : 0.0, my += on ? f.y : 0.0, mz += on ? f.z : 0.0;
  }
  if (v >= V) {
    return;
  }
  const V3 m{mx, my, mz};
  const double s = norm2(m);
  const double inv = 1.0 / sqrt(s);
  float nx = float(mx * inv), ny = float(my * inv), nz = float(mz * inv);
  if (s == 0.0) {
    nx = ny = nz = 0.f;
  } else if (!(fabs(s) <= 1.79769313486231570815e308)) {
    nx = ny = nz = __builtin_nanf("");
  }
  const size_t o = (size_t(b) * size_t(V) + size_t(v)) * 3;
  store3(normals + o, nx, ny, nz);
  if (sums != nullptr) {
    store3(sums + o, float(mx), float(my), float(mz));
  }
}

__global__ void __launch_bounds__(kMeshThreads) vertexNormalsBackwardKernel(
    MeshDev mesh,
    const float* __restrict__ positions, // [B][V][3]
    const float* __restrict__ sums, // [B][V][3] m_v of the forward
    const float* __restrict__ normalGrad, // [B][V][3]
    float* __restrict__ positionGrad) { // [B][V][3] every entry written
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int b = int(blockIdx.x) / mesh.tiles, tile = int(blockIdx.x) % mesh.tiles;
  const int group = tile * (kMeshThreads / kMeshGroup) + wave;
  if (group >= mesh.numGroups) {
    return;
  }
  const int V = mesh.V, v = group * kMeshGroup + lane;
  const size_t inst = size_t(b) * size_t(V) * 3;
  const float* p = positions + inst;
  const float* m = sums + inst;
  const float* g = normalGrad + inst;
  const int4* rec = mesh.records + size_t(mesh.groupBase[group]) + size_t(lane);
  const int rows = mesh.groupMax[group];
  double dx = 0.0, dy = 0.0, dz = 0.0;
#pragma unroll 1
  for (int i = 0; i < rows; ++i) {
    const int4 r = rec[size_t(i) * kMeshGroup];
    const size_t a3 = size_t(r.x) * 3, b3 = size_t(r.y) * 3, c3 = size_t(r.z) * 3;
    const size_t next = r.w == 0 ? b3 : (r.w == 1 ? c3 : a3), prev = r.w == 0 ? c3 : (r.w == 1 ? a3 : b3);
    const V3 pn = load3(p + next), pp = load3(p + prev);
    const V3 ha = hOf(m + a3, g + a3), hb = hOf(m + b3, g + b3), hc = hOf(m + c3, g + c3);
    const V3 H{(ha.x + hb.x) + hc.x, (ha.y + hb.y) + hc.y, (ha.z + hb.z) + hc.z};
    const V3 t = cross(V3{pn.x - pp.x, pn.y - pp.y, pn.z - pp.z}, H);
    const bool on = r.w >= 0;
    dx += on ? t.x : 0.0, dy += on ? t.y : 0.0, dz += on ? t.z : 0.0;
  }
  if (v >= V) {
    return;
  }
  store3(positionGrad + inst + size_t(v) * 3, float(dx), float(dy), float(dz));
}

} // namespace
} // namespace mmx

// A triangle mesh on a device (mmx_mesh_create): the uploaded incidence list of the vertex-normal kernels and the plain
// triangle list [T][3] that mmx_closest_points_on_mesh.hip streams
struct mmx_mesh {
  int32_t device = 0, V = 0, T = 0;
  void* records = nullptr;
  void* groups = nullptr; // groupBase [G] then groupMax [G]
  void* triangles = nullptr; // [T][3]
  int32_t numGroups = 0;
  ~mmx_mesh() {
    if (triangles != nullptr) {
      (void)hipFree(triangles);
    }
    if (records != nullptr) {
      (void)hipFree(records);
    }
    if (groups != nullptr) {
      (void)hipFree(groups);
    }
  }
  mmx::MeshDev dev(int32_t tiles) const {
    mmx::MeshDev d{};
    d.V = V, d.tiles = tiles, d.numGroups = numGroups;
    d.records = static_cast<const int4*>(records);
    d.groupBase = static_cast<const int32_t*>(groups);
    d.groupMax = d.groupBase + numGroups;
    return d;
  }
};

namespace mmx {
// what mmx_closest_points_on_mesh.hip reads of a handle
const int32_t* meshTriangleList(const mmx_mesh* mesh) {
  return static_cast<const int32_t*>(mesh->triangles);
}
int32_t meshDeviceOrdinal(const mmx_mesh* mesh) {
  return mesh->device;
}

namespace {

int32_t hipFail(const char* fn, const char* what, hipError_t e) {
  return failWith(e == hipErrorOutOfMemory ? MMX_ERR_OUT_OF_MEMORY : MMX_ERR_DEVICE, std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
}

// the checks of a batched call that need no device; null = fine
const char* callRefusal(int32_t V, int32_t batch, bool pointersOk, const char* pointers, int64_t* workgroups) {
  if (!pointersOk) {
    return pointers;
  }
  return meshBatchRefusal(V, batch, workgroups);
}

struct Buf { // (freed on every way out)
  void* p = nullptr;
  ~Buf() {
    if (p != nullptr) {
      (void)hipFree(p);
    }
  }
  hipError_t up(const void* host, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && host != nullptr) {
      e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
    }
    return e;
  }
  float* f() const {
    return static_cast<float*>(p);
  }
};

struct MeshDeleter {
  void operator()(mmx_mesh* m) const {
    mmx_mesh_destroy(m);
  }
};

} // namespace
} // namespace mmx

extern "C" {

int32_t mmx_host_mesh_tables(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t* vertex_start,
    int32_t* entry_triangle,
    int32_t* entry_corner,
    int32_t* num_entries,
    int32_t* max_valence) {
  std::string err;
  const int32_t rc = mmx::validateMesh(num_vertices, num_triangles, triangles, err);
  if (rc != MMX_OK) {
    return mmx::failWith(rc, "mmx_host_mesh_tables: " + err);
  }
  const mmx::MeshTables t = mmx::buildMeshTables(num_vertices, num_triangles, triangles, false);
  if (vertex_start != nullptr) {
    std::copy(t.vertexStart.begin(), t.vertexStart.end(), vertex_start);
  }
  if (entry_triangle != nullptr) {
    std::copy(t.entryTriangle.begin(), t.entryTriangle.end(), entry_triangle);
  }
  if (entry_corner != nullptr) {
    std::copy(t.entryCorner.begin(), t.entryCorner.end(), entry_corner);
  }
  if (num_entries != nullptr) {
    *num_entries = int32_t(t.entryTriangle.size());
  }
  if (max_valence != nullptr) {
    *max_valence = t.maxValence;
  }
  return MMX_OK;
}

int32_t mmx_mesh_create(int32_t num_vertices, int32_t num_triangles, const int32_t* triangles, int32_t device, mmx_mesh** out) {
  if (out == nullptr) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, "mmx_mesh_create: out is null");
  }
  *out = nullptr;
  std::string err;
  const int32_t rc = mmx::validateMesh(num_vertices, num_triangles, triangles, err);
  if (rc != MMX_OK) {
    return mmx::failWith(rc, "mmx_mesh_create: " + err);
  }
  const mmx::MeshTables t = mmx::buildMeshTables(num_vertices, num_triangles, triangles, true);
  if (!t.fits) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, "mmx_mesh_create: the incidence list, padded per 64 vertices to the group's highest valence, exceeds 2^31 - 1 records");
  }
  std::unique_ptr<mmx_mesh> m(new (std::nothrow) mmx_mesh());
  if (!m) {
    return mmx::failWith(MMX_ERR_OUT_OF_MEMORY, "mmx_mesh_create: out of host memory");
  }
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    return mmx::hipFail("mmx_mesh_create", "hipSetDevice", e);
  }
  m->device = device, m->V = num_vertices, m->T = num_triangles, m->numGroups = int32_t(t.groupBase.size());
  const size_t recBytes = std::max<size_t>(t.records.size(), 4) * sizeof(int32_t), grpBytes = size_t(m->numGroups) * sizeof(int32_t);
  e = hipMalloc(&m->records, recBytes);
  e = e != hipSuccess ? e : hipMalloc(&m->groups, 2 * grpBytes);
  const size_t triBytes = size_t(num_triangles) * 3 * sizeof(int32_t);
  e = e != hipSuccess ? e : hipMalloc(&m->triangles, triBytes);
  e = e != hipSuccess ? e : hipMemcpy(m->triangles, triangles, triBytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && !t.records.empty()) {
    e = hipMemcpy(m->records, t.records.data(), t.records.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  }
  e = e != hipSuccess ? e : hipMemcpy(m->groups, t.groupBase.data(), grpBytes, hipMemcpyHostToDevice);
  e = e != hipSuccess ? e : hipMemcpy(static_cast<char*>(m->groups) + grpBytes, t.groupMax.data(), grpBytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    return mmx::hipFail("mmx_mesh_create", "upload", e);
  }
  *out = m.release();
  return MMX_OK;
}

void mmx_mesh_destroy(mmx_mesh* mesh) {
  if (mesh != nullptr) {
    (void)hipSetDevice(mesh->device);
    delete mesh;
  }
}

int32_t mmx_mesh_num_vertices(const mmx_mesh* mesh) {
  return mesh ? mesh->V : 0;
}

int32_t mmx_mesh_num_triangles(const mmx_mesh* mesh) {
  return mesh ? mesh->T : 0;
}

int32_t mmx_vertex_normals(mmx_mesh* mesh, int32_t batch, const float* positions_dev, float* normals_dev, float* sums_dev, void* stream) {
  int64_t workgroups = 0;
  if (const char* why = mmx::callRefusal(
          mesh ? mesh->V : 1, batch, mesh != nullptr && positions_dev != nullptr && normals_dev != nullptr, "mesh / positions / normals is null",
          &workgroups)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string("mmx_vertex_normals: ") + why);
  }
  hipError_t e = hipSetDevice(mesh->device);
  if (e != hipSuccess) {
    return mmx::hipFail("mmx_vertex_normals", "hipSetDevice", e);
  }
  hipLaunchKernelGGL(
      mmx::vertexNormalsKernel, dim3(unsigned(workgroups)), dim3(mmx::kMeshThreads), 0, static_cast<hipStream_t>(stream),
      mesh->dev(int32_t(workgroups / batch)), positions_dev, normals_dev, sums_dev);
  e = hipGetLastError();
  if (e != hipSuccess) {
    return mmx::hipFail("mmx_vertex_normals", "launch", e);
  }
  return MMX_OK;
}

int32_t mmx_vertex_normals_backward(
    mmx_mesh* mesh,
    int32_t batch,
    const float* positions_dev,
    const float* sums_dev,
    const float* normal_grad_dev,
    float* position_grad_dev,
    void* stream) {
  int64_t workgroups = 0;
  const bool ok = mesh != nullptr && positions_dev != nullptr && sums_dev != nullptr && normal_grad_dev != nullptr && position_grad_dev != nullptr;
  if (const char* why = mmx::callRefusal(mesh ? mesh->V : 1, batch, ok, "mesh / positions / sums / normal_grad / position_grad is null", &workgroups)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string("mmx_vertex_normals_backward: ") + why);
  }
  hipError_t e = hipSetDevice(mesh->device);
  if (e != hipSuccess) {
    return mmx::hipFail("mmx_vertex_normals_backward", "hipSetDevice", e);
  }
  hipLaunchKernelGGL(
      mmx::vertexNormalsBackwardKernel, dim3(unsigned(workgroups)), dim3(mmx::kMeshThreads), 0, static_cast<hipStream_t>(stream),
      mesh->dev(int32_t(workgroups / batch)), positions_dev, sums_dev, normal_grad_dev, position_grad_dev);
  e = hipGetLastError();
  if (e != hipSuccess) {
    return mmx::hipFail("mmx_vertex_normals_backward", "launch", e);
  }
  return MMX_OK;
}

int32_t mmx_vertex_normals_host(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t device,
    int32_t batch,
    const float* positions_host,
    float* normals_host,
    float* sums_host) {
  const char* fn = "mmx_vertex_normals_host";
  std::string err;
  if (mmx::validateMesh(num_vertices, num_triangles, triangles, err) != MMX_OK) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + err);
  }
  if (const char* why = mmx::callRefusal(num_vertices, batch, positions_host != nullptr && normals_host != nullptr, "positions / normals is null", nullptr)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + why);
  }
  mmx_mesh* raw = nullptr;
  int32_t rc = mmx_mesh_create(num_vertices, num_triangles, triangles, device, &raw);
  if (rc != MMX_OK) {
    return rc;
  }
  std::unique_ptr<mmx_mesh, mmx::MeshDeleter> mesh(raw);
  const size_t bytes = size_t(batch) * size_t(num_vertices) * 3 * sizeof(float);
  mmx::Buf pos, nrm, sum;
  hipError_t e = pos.up(positions_host, bytes);
  e = e != hipSuccess ? e : nrm.up(nullptr, bytes);
  if (sums_host != nullptr) {
    e = e != hipSuccess ? e : sum.up(nullptr, bytes);
  }
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "upload", e);
  }
  rc = mmx_vertex_normals(mesh.get(), batch, pos.f(), nrm.f(), sum.f(), nullptr);
  if (rc != MMX_OK) {
    return rc;
  }
  e = hipDeviceSynchronize();
  e = e != hipSuccess ? e : hipMemcpy(normals_host, nrm.p, bytes, hipMemcpyDeviceToHost);
  if (sums_host != nullptr) {
    e = e != hipSuccess ? e : hipMemcpy(sums_host, sum.p, bytes, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "download", e);
  }
  return MMX_OK;
}

int32_t mmx_vertex_normals_backward_host(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t device,
    int32_t batch,
    const float* positions_host,
    const float* sums_host,
    const float* normal_grad_host,
    float* position_grad_host) {
  const char* fn = "mmx_vertex_normals_backward_host";
  std::string err;
  if (mmx::validateMesh(num_vertices, num_triangles, triangles, err) != MMX_OK) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + err);
  }
  const bool ok = positions_host != nullptr && sums_host != nullptr && normal_grad_host != nullptr && position_grad_host != nullptr;
  if (const char* why = mmx::callRefusal(num_vertices, batch, ok, "positions / sums / normal_grad / position_grad is null", nullptr)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + why);
  }
  mmx_mesh* raw = nullptr;
  int32_t rc = mmx_mesh_create(num_vertices, num_triangles, triangles, device, &raw);
  if (rc != MMX_OK) {
    return rc;
  }
  std::unique_ptr<mmx_mesh, mmx::MeshDeleter> mesh(raw);
  const size_t bytes = size_t(batch) * size_t(num_vertices) * 3 * sizeof(float);
  mmx::Buf pos, sum, grad, out;
  hipError_t e = pos.up(positions_host, bytes);
  e = e != hipSuccess ? e : sum.up(sums_host, bytes);
  e = e != hipSuccess ? e : grad.up(normal_grad_host, bytes);
  e = e != hipSuccess ? e : out.up(nullptr, bytes);
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "upload", e);
  }
  rc = mmx_vertex_normals_backward(mesh.get(), batch, pos.f(), sum.f(), grad.f(), out.f(), nullptr);
  if (rc != MMX_OK) {
    return rc;
  }
  e = hipDeviceSynchronize();
  e = e != hipSuccess ? e : hipMemcpy(position_grad_host, out.p, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "download", e);
  }
  return MMX_OK;
}

} // extern "C"
