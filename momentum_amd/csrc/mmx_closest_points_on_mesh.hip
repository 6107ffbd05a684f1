// mmx_closest_points_on_mesh.hip -- closest points ON a posed triangle mesh (gfx950 / CDNA4, wave64): for every source point
// of every instance, the nearest point of the nearest eligible triangle of that instance's mesh, with its face index and
// barycentric coordinates (include/mmx.h: mmx_closest_points_on_mesh).  The counterpart of
// pymomentum.geometry.find_closest_points_on_mesh, which runs on the CPU.  The kernel, its launcher and the three C-ABI entry
// points live here; the launch decision is mmx_closest_points_on_mesh_plan.cpp; the handle is mmx_vertex_normals.hip's.
//
// Two functions hold the arithmetic and every use goes through them (no contraction is left to the compiler):
//   triangleRecord   a, e1 = b - a, e2 = c - a, the Gram terms d11, d12, d22 and the three reciprocals the pair wants hoisted
//                    (1 / d11, 1 / d22, 1 / |b - c|^2: the edges' own); all NaN for an ineligible triangle
//   pairOnTriangle   v = p - a first, Ericson's regions with selects, clamps, then dist2 = |v - s e1 - t e2|^2 of the
//                    residual vector; two sources at a time so that the packed f32 instructions are in hand
//
// closestPointsOnMeshKernel has the shape of closestPointsKernel (mmx_closest_points.hip).  A 256-thread workgroup works on
// one instance; a lane owns a register block of four sources 64 apart (coordinates, best dist2, best face).  The instance's
// triangles stream through LDS as tiles of 256 RECORDS, structure of arrays (15 arrays of 256 floats): thread i reads triangle
// t0 + i's three indices from the handle's list, gathers the three posed vertices and computes the record into registers
// BEFORE it scans the current tile, and stores it into the other buffer after, one barrier per tile.  Wave w scans the w-th
// quarter of every tile: all lanes read the same address, a broadcast, one ds_read_b128 per array brings four triangles,
// then 4 triangles x 4 sources = 16 pairs.  Faces are taken in ascending order with a strict <, so within a lane the lowest
// index wins among equal dist2.  Only (dist2, face) is kept in the loop; max_dist is applied once, at the end (the smallest
// finite dist2 is the eligible minimum when it is <= max_dist^2 and otherwise nothing is).  The remainder of the last tile
// is NaN records, whose dist2 is NaN and never < anything: it runs the same loop body.  A source past N is NaN as well.
// The four partial (dist2, face) per source meet in LDS and a thread takes a source's lexicographic minimum over w = 0..3;
// it then recomputes the winning pair through the same two functions -- the same bits -- for s, t and the point.
// No atomics, no scratch; an instance reads no other instance's data.
//
// LDS map (floats): buf[2][15][256] (30 KB), then partD2[4][256], partFace[4][256] (8 KB).  38 KB in all.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <string>

#include "../../include/mmx.h"
#include "mmx_closest_points_on_mesh_plan.hpp"
#include "mmx_mesh_tables.hpp"

namespace mmx {
int32_t failWith(int32_t code, const std::string& msg); // mmx_capi.hip: sets mmx_last_error()
const int32_t* meshTriangleList(const mmx_mesh* mesh); // mmx_vertex_normals.hip: the handle's [T][3] list on its device
int32_t meshDeviceOrdinal(const mmx_mesh* mesh);

namespace {

struct ClosestPointsOnMeshArgs {
  int32_t N, T, groups /* workgroups per instance */;
  const int32_t* triangles; // [T][3]
  const float* source; // [B][N][3]
  const float* vertices; // [B][V][3] or [V][3]
  size_t vertexStride; // floats between two instances' vertices (0: shared)
  float maxDist2;
  int32_t* face; // [B][N]
  float* barycentric; // null or [B][N][3]
  float* points; // null or [B][N][3]
  float* dist2; // null or [B][N]
};

typedef float float2v __attribute__((ext_vector_type(2)));

// a triangle's record: kCpmRecord floats, always indexed by these constants (so that it lives in registers)
enum : int { kAx, kAy, kAz, kE1x, kE1y, kE1z, kE2x, kE2y, kE2z, kD11, kD12, kD22, kI11, kI22, kIbc, kRecordEnd };
static_assert(kRecordEnd == kCpmRecord, "the record is kCpmRecord floats");
typedef float TriRecord[kCpmRecord];

__device__ __forceinline__ float dot3(float ux, float uy, float uz, float wx, float wy, float wz) {
#pragma clang fp contract(off)
  return __builtin_fmaf(uz, wz, __builtin_fmaf(uy, wy, ux * wx));
}
__device__ __forceinline__ float2v dot3(float ux, float uy, float uz, float2v wx, float2v wy, float2v wz) {
#pragma clang fp contract(off)
  const float2v x = ux, y = uy, z = uz;
  return __builtin_elementwise_fma(z, wz, __builtin_elementwise_fma(y, wy, x * wx));
}
__device__ __forceinline__ bool finite(float x) {
  return __builtin_fabsf(x) <= 3.40282346638528859812e38f;
}

// THE record of a triangle: every copy goes through this sequence and no other.  All NaN when the triangle is ineligible
// (a face vector of three exact zeros, or a value that is not finite).
__device__ __forceinline__ void triangleRecord(const float* a, const float* b, const float* c, TriRecord& o) {
#pragma clang fp contract(off)
  const float ax = a[0], ay = a[1], az = a[2];
  const float e1x = b[0] - ax, e1y = b[1] - ay, e1z = b[2] - az;
  const float e2x = c[0] - ax, e2y = c[1] - ay, e2z = c[2] - az;
  // both products of a component rounded, then the difference: u x u is three exact zeros
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float d11 = dot3(e1x, e1y, e1z, e1x, e1y, e1z);
  const float d12 = dot3(e2x, e2y, e2z, e1x, e1y, e1z);
  const float d22 = dot3(e2x, e2y, e2z, e2x, e2y, e2z);
  const float i11 = 1.f / d11;
  const float i22 = 1.f / d22;
  const float ibc = 1.f / ((d11 - d12) + (d22 - d12));
  bool ok = !(nx == 0.f && ny == 0.f && nz == 0.f);
  ok = ok && finite(ax) && finite(ay) && finite(az) && finite(e1x) && finite(e1y) && finite(e1z) && finite(e2x) && finite(e2y) && finite(e2z) &&
      finite(d11) && finite(d12) && finite(d22) && finite(i11) && finite(i22) && finite(ibc);
  const float kNaN = __builtin_nanf("");
  o[kAx] = ok ? ax : kNaN, o[kAy] = ok ? ay : kNaN, o[kAz] = ok ? az : kNaN;
  o[kE1x] = ok ? e1x : kNaN, o[kE1y] = ok ? e1y : kNaN, o[kE1z] = ok ? e1z : kNaN;
  o[kE2x] = ok ? e2x : kNaN, o[kE2y] = ok ? e2y : kNaN, o[kE2z] = ok ? e2z : kNaN;
  o[kD11] = ok ? d11 : kNaN, o[kD12] = ok ? d12 : kNaN, o[kD22] = ok ? d22 : kNaN;
  o[kI11] = ok ? i11 : kNaN, o[kI22] = ok ? i22 : kNaN, o[kIbc] = ok ? ibc : kNaN;
}

struct PairResult {
  float2v s, t, d2;
};

// the region selects of one pair, in reverse order of priority: the last that applies wins
__device__ __forceinline__ void regionSelect(
    float d1, float d2, float d3, float d4, float d5, float d6, float va, float vb, float vc, float e43, float e56, float w, float omw, float sAB,
    float tAC, float& s, float& t) {
  const bool bc = va <= 0.f && e43 >= 0.f && e56 >= 0.f;
  s = bc ? omw : s, t = bc ? w : t;
  const bool ac = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
  s = ac ? 0.f : s, t = ac ? tAC : t;
  const bool c = d6 >= 0.f && d5 <= d6;
  s = c ? 0.f : s, t = c ? 1.f : t;
  const bool ab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
  s = ab ? sAB : s, t = ab ? 0.f : t;
  const bool b = d3 >= 0.f && d4 <= d3;
  s = b ? 1.f : s, t = b ? 0.f : t;
  const bool a = d1 <= 0.f && d2 <= 0.f;
  s = a ? 0.f : s, t = a ? 0.f : t;
}

// THE pair: every (source, triangle) goes through this sequence and no other, two sources at a time (each half of a packed
// instruction is the IEEE operation of the unpacked one: the same bits)
__device__ __forceinline__ PairResult pairOnTriangle(float2v px, float2v py, float2v pz, const TriRecord& k) {
#pragma clang fp contract(off)
  const float2v vx = px - k[kAx], vy = py - k[kAy], vz = pz - k[kAz];
  const float2v d1 = dot3(k[kE1x], k[kE1y], k[kE1z], vx, vy, vz), d2 = dot3(k[kE2x], k[kE2y], k[kE2z], vx, vy, vz);
  const float2v d3 = d1 - k[kD11], d4 = d2 - k[kD12], d5 = d1 - k[kD12], d6 = d2 - k[kD22];
  const float2v vc = __builtin_elementwise_fma(d1, d4, -(d3 * d2));
  const float2v vb = __builtin_elementwise_fma(d5, d2, -(d1 * d6));
  const float2v va = __builtin_elementwise_fma(d3, d6, -(d5 * d4));
  // the interior: normalised by the pair's OWN va + vb + vc (the hardware reciprocal, within a unit in the last place), not by a
  // hoisted 1 / |e1 x e2|^2 -- on a sliver the three carry the same cancellation error, so their ratios stay sound where a
  // hoisted determinant does not (measured: 23 u R against 5000 u R on posed meshes with slivers)
  const float2v sum = (va + vb) + vc;
  const float2v den{__builtin_amdgcn_rcpf(sum.x), __builtin_amdgcn_rcpf(sum.y)};
  const float2v sIn = vb * den, tIn = vc * den;
  const float2v e43 = d4 - d3, e56 = d5 - d6;
  const float2v w = e43 * k[kIbc], omw = 1.f - w;
  const float2v sAB = d1 * k[kI11], tAC = d2 * k[kI22];
  float s0 = sIn.x, t0 = tIn.x, s1 = sIn.y, t1 = tIn.y;
  regionSelect(d1.x, d2.x, d3.x, d4.x, d5.x, d6.x, va.x, vb.x, vc.x, e43.x, e56.x, w.x, omw.x, sAB.x, tAC.x, s0, t0);
  regionSelect(d1.y, d2.y, d3.y, d4.y, d5.y, d6.y, va.y, vb.y, vc.y, e43.y, e56.y, w.y, omw.y, sAB.y, tAC.y, s1, t1);
  const float2v zero = 0.f, one = 1.f;
  // clamped, then rounded to a multiple of 2^-24 by 1 - (1 - x): 1 - x is such a multiple in [0.5, 1] or exact, and the outer
  // subtraction is exact.  1 - s and (1 - s) - t are then exact, so the three weights sum to 1 with no rounding at all.
  const float2v os = one - __builtin_elementwise_min(__builtin_elementwise_max(float2v{s0, s1}, zero), one);
  const float2v s = one - os;
  const float2v t = one - (one - __builtin_elementwise_min(__builtin_elementwise_max(float2v{t0, t1}, zero), os));
  const float2v e1x = k[kE1x], e1y = k[kE1y], e1z = k[kE1z], e2x = k[kE2x], e2y = k[kE2y], e2z = k[kE2z];
  const float2v rx = __builtin_elementwise_fma(-t, e2x, __builtin_elementwise_fma(-s, e1x, vx));
  const float2v ry = __builtin_elementwise_fma(-t, e2y, __builtin_elementwise_fma(-s, e1y, vy));
  const float2v rz = __builtin_elementwise_fma(-t, e2z, __builtin_elementwise_fma(-s, e1z, vz));
  PairResult out;
  out.s = s, out.t = t;
  out.d2 = __builtin_elementwise_fma(rz, rz, __builtin_elementwise_fma(ry, ry, rx * rx));
  return out;
}

__device__ __forceinline__ float comp(const float4& v, int j) {
  return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w));
}

__global__ void __launch_bounds__(kCpmThreads) closestPointsOnMeshKernel(ClosestPointsOnMeshArgs a) {
  constexpr int T = kCpmTile, C = kCpmRecord;
  static_assert(T == kCpmThreads && (T / kCpmWays) % 4 == 0, "a thread stages one record per tile; a wave's share is whole groups of four");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* partD2 = smem + 2 * C * T;
  int32_t* partFace = reinterpret_cast<int32_t*>(partD2 + kCpmWays * kCpmWaveSources);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int b = int(blockIdx.x) / a.groups, g = int(blockIdx.x) % a.groups;
  const int N = a.N, numTri = a.T;
  const float kNaN = __builtin_nanf("");
  const float kInf = __builtin_inff();

  // ---- this lane's sources
  const int sBase = g * kCpmWaveSources;
  const float* srcB = a.source + size_t(b) * size_t(N) * 3;
  float sx[kCpmBlock], sy[kCpmBlock], sz[kCpmBlock], best[kCpmBlock];
  int32_t bestFace[kCpmBlock];
#pragma unroll
  for (int r = 0; r < kCpmBlock; ++r) {
    const int s = sBase + 64 * r + lane;
    const bool in = s < N;
    const size_t o = in ? size_t(s) * 3 : 0;
    sx[r] = in ? srcB[o] : kNaN, sy[r] = in ? srcB[o + 1] : kNaN, sz[r] = in ? srcB[o + 2] : kNaN;
    best[r] = kInf, bestFace[r] = -1;
  }

  // ---- the triangles, tile by tile
  const float* vtxB = a.vertices + size_t(b) * a.vertexStride;
  auto recordOf = [&](int t, TriRecord& o) { // (t < numTri) global -> the record
    const int32_t* tri = a.triangles + size_t(t) * 3;
    const int32_t ia = tri[0], ib = tri[1], ic = tri[2];
    triangleRecord(vtxB + size_t(ia) * 3, vtxB + size_t(ib) * 3, vtxB + size_t(ic) * 3, o);
  };
  TriRecord stage;
  auto loadTile = [&](int t0) { // past the list's end: a NaN record
    const int t = t0 + tid;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      stage[c] = kNaN;
    }
    if (t < numTri) {
      recordOf(t, stage);
    }
  };
  auto storeTile = [&](float* buf) { // registers -> LDS, structure of arrays
#pragma unroll
    for (int c = 0; c < C; ++c) {
      buf[c * T + tid] = stage[c];
    }
  };
  const int numTiles = (numTri + T - 1) / T;
  loadTile(0);
  storeTile(smem);
  __syncthreads();
#pragma unroll 1
  for (int tile = 0; tile < numTiles; ++tile) {
    const int t0 = tile * T;
    const float* buf = smem + (tile & 1) * C * T;
    const bool more = tile + 1 < numTiles;
    if (more) {
      loadTile(t0 + T);
    }
    // this wave's share of the tile, whole groups of four (the padding inside the last group is NaN)
    const int count = (min(T, numTri - t0) + 3) & ~3;
    const int lo = wave * (T / kCpmWays);
    const int hi = min(lo + T / kCpmWays, count);
#pragma unroll 1
    for (int t = lo; t < hi; t += 4) {
      float4 q[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        q[c] = *reinterpret_cast<const float4*>(buf + c * T + t);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int32_t ti = t0 + t + j;
        TriRecord k;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          k[c] = comp(q[c], j);
        }
#pragma unroll
        for (int r = 0; r < kCpmBlock; r += 2) {
          const PairResult p = pairOnTriangle(float2v{sx[r], sx[r + 1]}, float2v{sy[r], sy[r + 1]}, float2v{sz[r], sz[r + 1]}, k);
          const bool take0 = p.d2.x < best[r], take1 = p.d2.y < best[r + 1]; // ordered: false for NaN, and for +inf against the initial +inf
          best[r] = take0 ? p.d2.x : best[r], best[r + 1] = take1 ? p.d2.y : best[r + 1];
          bestFace[r] = take0 ? ti : bestFace[r], bestFace[r + 1] = take1 ? ti : bestFace[r + 1];
        }
      }
    }
    if (more) {
      storeTile(smem + ((tile + 1) & 1) * C * T);
    }
    __syncthreads();
  }

  // ---- results: the four partials of a source, max_dist once, then every entry of every output
#pragma unroll
  for (int r = 0; r < kCpmBlock; ++r) {
    partD2[wave * kCpmWaveSources + 64 * r + lane] = best[r];
    partFace[wave * kCpmWaveSources + 64 * r + lane] = bestFace[r];
  }
  __syncthreads();
#pragma unroll
  for (int local = tid; local < kCpmWaveSources; local += kCpmThreads) { // (one source per thread with a block of four)
    const int s = sBase + local;
    if (s < N) {
      float d2 = partD2[local];
      int32_t f = partFace[local];
#pragma unroll
      for (int w = 1; w < kCpmWays; ++w) {
        const float dw = partD2[w * kCpmWaveSources + local];
        const int32_t fw = partFace[w * kCpmWaveSources + local];
        const bool take = fw >= 0 && (dw < d2 || (dw == d2 && fw < f)); // (d2 == +inf only with f == -1, and then dw < d2)
        d2 = take ? dw : d2, f = take ? fw : f;
      }
      const bool valid = f >= 0 && d2 <= a.maxDist2;
      const size_t o = size_t(b) * size_t(N) + size_t(s);
      a.face[o] = valid ? f : -1;
      if (a.dist2 != nullptr) {
        a.dist2[o] = valid ? d2 : kInf;
      }
      if (a.barycentric != nullptr || a.points != nullptr) {
        // the winning pair again, through the same two functions: the same bits (triangle 0 exists: T >= 1)
        TriRecord k;
        recordOf(valid ? f : 0, k);
        const float px = srcB[size_t(s) * 3], py = srcB[size_t(s) * 3 + 1], pz = srcB[size_t(s) * 3 + 2];
        const PairResult p = pairOnTriangle(float2v{px, px}, float2v{py, py}, float2v{pz, pz}, k);
        const float ws = p.s.x, wt = p.t.x;
        if (a.barycentric != nullptr) {
          const float wa = (1.f - ws) - wt;
          a.barycentric[3 * o] = valid ? wa : 0.f, a.barycentric[3 * o + 1] = valid ? ws : 0.f, a.barycentric[3 * o + 2] = valid ? wt : 0.f;
        }
        if (a.points != nullptr) {
          const float qx = __builtin_fmaf(wt, k[kE2x], __builtin_fmaf(ws, k[kE1x], k[kAx]));
          const float qy = __builtin_fmaf(wt, k[kE2y], __builtin_fmaf(ws, k[kE1y], k[kAy]));
          const float qz = __builtin_fmaf(wt, k[kE2z], __builtin_fmaf(ws, k[kE1z], k[kAz]));
          a.points[3 * o] = valid ? qx : 0.f, a.points[3 * o + 1] = valid ? qy : 0.f, a.points[3 * o + 2] = valid ? qz : 0.f;
        }
      }
    }
  }
}
static_assert(kCpmBlock % 2 == 0 && kCpmWaveSources % kCpmThreads == 0, "sources go two at a time; the last step finishes whole passes of the workgroup");

size_t closestPointsOnMeshLdsBytes() {
  return (2 * size_t(kCpmRecord) * kCpmTile + 2 * size_t(kCpmWays) * kCpmWaveSources) * sizeof(float);
}

// the checks every entry point makes before anything is touched; null = fine
const char* closestPointsOnMeshRefusal(
    int32_t batch, int32_t N, int32_t T, bool pointersOk, const char* pointers, float maxDist, ClosestPointsOnMeshPlan* plan) {
  if (!pointersOk) {
    return pointers;
  }
  if (batch < 1 || N < 1) {
    return "batch and num_source must be >= 1";
  }
  if (!(maxDist >= 0.f)) {
    return "max_dist must be >= 0 (+inf allowed), not negative or NaN";
  }
  if (!closestPointsOnMeshPlan(batch, N, T, plan)) {
    return "the launch grid exceeds 2^31 - 1 workgroups";
  }
  return nullptr;
}

int32_t hipFail(const char* fn, const char* what, hipError_t e) {
  return failWith(e == hipErrorOutOfMemory ? MMX_ERR_OUT_OF_MEMORY : MMX_ERR_DEVICE, std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
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

int32_t mmx_closest_points_on_mesh_plan(
    int32_t batch, int32_t num_source, int32_t num_triangles, int32_t* sources_per_workgroup, int32_t* triangle_tile, int32_t* triangle_ways) {
  mmx::ClosestPointsOnMeshPlan p;
  if (!mmx::closestPointsOnMeshPlan(batch, num_source, num_triangles, &p)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, "mmx_closest_points_on_mesh_plan: a size below 1, or a launch grid beyond 2^31 - 1 workgroups");
  }
  if (sources_per_workgroup != nullptr) {
    *sources_per_workgroup = p.sourcesPerWorkgroup;
  }
  if (triangle_tile != nullptr) {
    *triangle_tile = p.triangleTile;
  }
  if (triangle_ways != nullptr) {
    *triangle_ways = p.triangleWays;
  }
  return MMX_OK;
}

int32_t mmx_closest_points_on_mesh(
    mmx_mesh* mesh,
    int32_t batch,
    int32_t num_source,
    const float* source_dev,
    const float* vertices_dev,
    int32_t vertices_shared,
    float max_dist,
    int32_t* face_index_dev,
    float* barycentric_dev,
    float* points_dev,
    float* dist2_dev,
    void* stream) {
  const char* fn = "mmx_closest_points_on_mesh";
  mmx::ClosestPointsOnMeshPlan plan;
  const bool ok = mesh != nullptr && source_dev != nullptr && vertices_dev != nullptr && face_index_dev != nullptr;
  if (const char* why = mmx::closestPointsOnMeshRefusal(
          batch, num_source, mesh ? mmx_mesh_num_triangles(mesh) : 1, ok, "mesh / source / vertices / face_index is null", max_dist, &plan)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + why);
  }
  hipError_t e = hipSetDevice(mmx::meshDeviceOrdinal(mesh));
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "hipSetDevice", e);
  }
  mmx::ClosestPointsOnMeshArgs a{};
  a.N = num_source, a.T = mmx_mesh_num_triangles(mesh), a.groups = int32_t(plan.workgroups / batch);
  a.triangles = mmx::meshTriangleList(mesh);
  a.source = source_dev, a.vertices = vertices_dev;
  a.vertexStride = vertices_shared != 0 ? 0 : size_t(mmx_mesh_num_vertices(mesh)) * 3;
  a.maxDist2 = max_dist * max_dist; // (float32: +inf stays +inf)
  a.face = face_index_dev, a.barycentric = barycentric_dev, a.points = points_dev, a.dist2 = dist2_dev;
  hipLaunchKernelGGL(
      mmx::closestPointsOnMeshKernel, dim3(unsigned(plan.workgroups)), dim3(mmx::kCpmThreads), mmx::closestPointsOnMeshLdsBytes(),
      static_cast<hipStream_t>(stream), a);
  e = hipGetLastError();
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "launch", e);
  }
  return MMX_OK;
}

int32_t mmx_closest_points_on_mesh_host(
    int32_t num_vertices,
    int32_t num_triangles,
    const int32_t* triangles,
    int32_t device,
    int32_t batch,
    int32_t num_source,
    const float* source_host,
    const float* vertices_host,
    int32_t vertices_shared,
    float max_dist,
    int32_t* face_index_host,
    float* barycentric_host,
    float* points_host,
    float* dist2_host) {
  const char* fn = "mmx_closest_points_on_mesh_host";
  std::string err;
  if (mmx::validateMesh(num_vertices, num_triangles, triangles, err) != MMX_OK) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + err);
  }
  mmx::ClosestPointsOnMeshPlan plan;
  const bool ok = source_host != nullptr && vertices_host != nullptr && face_index_host != nullptr;
  if (const char* why =
          mmx::closestPointsOnMeshRefusal(batch, num_source, num_triangles, ok, "source / vertices / face_index is null", max_dist, &plan)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + why);
  }
  mmx_mesh* raw = nullptr;
  int32_t rc = mmx_mesh_create(num_vertices, num_triangles, triangles, device, &raw);
  if (rc != MMX_OK) {
    return rc;
  }
  std::unique_ptr<mmx_mesh, mmx::MeshDeleter> mesh(raw);
  const size_t nSrc = size_t(batch) * size_t(num_source);
  const size_t nVtx = (vertices_shared != 0 ? size_t(1) : size_t(batch)) * size_t(num_vertices);
  mmx::Buf src, vtx, face, bary, pts, d2;
  hipError_t e = src.up(source_host, nSrc * 3 * sizeof(float));
  e = e != hipSuccess ? e : vtx.up(vertices_host, nVtx * 3 * sizeof(float));
  e = e != hipSuccess ? e : face.up(nullptr, nSrc * sizeof(int32_t));
  if (barycentric_host != nullptr) {
    e = e != hipSuccess ? e : bary.up(nullptr, nSrc * 3 * sizeof(float));
  }
  if (points_host != nullptr) {
    e = e != hipSuccess ? e : pts.up(nullptr, nSrc * 3 * sizeof(float));
  }
  if (dist2_host != nullptr) {
    e = e != hipSuccess ? e : d2.up(nullptr, nSrc * sizeof(float));
  }
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "upload", e);
  }
  rc = mmx_closest_points_on_mesh(
      mesh.get(), batch, num_source, src.f(), vtx.f(), vertices_shared, max_dist, static_cast<int32_t*>(face.p), bary.f(), pts.f(), d2.f(), nullptr);
  if (rc != MMX_OK) {
    return rc;
  }
  e = hipDeviceSynchronize();
  e = e != hipSuccess ? e : hipMemcpy(face_index_host, face.p, nSrc * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (barycentric_host != nullptr) {
    e = e != hipSuccess ? e : hipMemcpy(barycentric_host, bary.p, nSrc * 3 * sizeof(float), hipMemcpyDeviceToHost);
  }
  if (points_host != nullptr) {
    e = e != hipSuccess ? e : hipMemcpy(points_host, pts.p, nSrc * 3 * sizeof(float), hipMemcpyDeviceToHost);
  }
  if (dist2_host != nullptr) {
    e = e != hipSuccess ? e : hipMemcpy(dist2_host, d2.p, nSrc * sizeof(float), hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    return mmx::hipFail(fn, "download", e);
  }
  return MMX_OK;
}

} // extern "C"
