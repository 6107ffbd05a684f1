// mmx_closest_points.hip -- batched nearest-point queries (gfx950 / CDNA4, wave64): for every source point of every
// instance, the eligible target of the same instance with the smallest squared distance (include/mmx.h: mmx_closest_points).
// The counterpart of pymomentum.geometry.find_closest_points, which runs on the CPU.  The kernel, its launcher and the three
// C-ABI entry points live here; the launch decision is mmx_closest_points_plan.cpp.
//
//   d2(s, t) = fma(dz, dz, fma(dy, dy, dx * dx)),   dx = s.x - t.x, dy = s.y - t.y, dz = s.z - t.z      (pairDist2, one place)
//
// closestPointsKernel<kNormals>.  A 256-thread workgroup works on one instance.  A lane owns a register block of four
// sources 64 apart (coordinates, best d2, best index; with normals their normals too).  The instance's targets stream through
// LDS as structure-of-arrays tiles of T targets (1024; 512 with normals): every thread loads the NEXT tile's 12 (or 2 x 6)
// floats from global memory into registers before it scans the current tile and stores them into the other buffer after it,
// one barrier per tile.  In the scan all lanes read the same address, a broadcast without bank conflict: one ds_read_b128
// per coordinate brings four targets, then 4 targets x 4 sources = 16 pairs, two sources at a time in packed instructions:
//     per two pairs 3 v_pk_add, 1 v_pk_mul, 2 v_pk_fma, then per pair 1 v_cmp (ordered <) and 2 v_cndmask
//     (with normals + 1 v_pk_mul, 2 v_pk_fma per two pairs and 1 v_cmp, 1 s_and per pair)
// -- 6.5 vector instructions per pair in the compiled loop, 9.2 with normals.
// Targets are taken in ascending order with a strict <, so within a lane the lowest index wins among equal d2.  max_dist is
// not in the loop: the smallest finite d2 over the targets that pass the normal test is the eligible minimum when it is
// <= max_dist^2 and otherwise nothing is eligible, so the bound is applied once, at the end.  The remainder of the last
// tile is padded with NaN coordinates, whose d2 is NaN and never < anything: it runs the same loop body.  A source past N is
// NaN as well.
//
// The four waves of a workgroup hold the SAME 256 sources and wave w scans the w-th quarter of every tile, so a launch has
// batch x ceil(N / 256) workgroups however small N is; the four partial (d2, index) per source meet in LDS and a thread takes
// a source's lexicographic minimum over w = 0..3 (d2 first, then the lower index; an empty partial is (+inf, -1) and never
// wins against a finite d2).
// No atomics, no scratch; an instance reads no other instance's data.
//
// LDS map (floats): buf[2][C][T] with C = 3 (x, y, z) or 6 (+ nx, ny, nz): 24 KB; then partD2[4][256], partIndex[4][256]
// (8 KB).  32 KB in all.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <string>

#include "../../include/mmx.h"
#include "mmx_closest_points_plan.hpp"

namespace mmx {
int32_t failWith(int32_t code, const std::string& msg); // mmx_capi.hip: sets mmx_last_error()

namespace {

struct ClosestPointsArgs {
  int32_t N, M, groups /* workgroups per instance */;
  const float* source; // [B][N][3]
  const float* target; // [B][M][3] or [M][3]
  const float* sourceNormals; // [B][N][3] (kNormals)
  const float* targetNormals; // like target (kNormals)
  size_t targetStride; // floats between two instances' targets (0: shared)
  float maxDist2, minNormalDot;
  int32_t* index; // [B][N]
  float* dist2; // null or [B][N]
  float* points; // null or [B][N][3]
};

// THE squared distance: every pair goes through this sequence and no other.  Two sources at a time, so that the compiler
// has v_pk_add / v_pk_mul / v_pk_fma in hand (each half is the IEEE operation of the unpacked instruction: the same bits).
typedef float float2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2v pairDist2(float2v sx, float2v sy, float2v sz, float tx, float ty, float tz) {
  const float2v dx = sx - tx, dy = sy - ty, dz = sz - tz;
  return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
}
__device__ __forceinline__ float2v pairDot(float2v ax, float2v ay, float2v az, float bx, float by, float bz) {
  const float2v x = bx, y = by, z = bz;
  return __builtin_elementwise_fma(az, z, __builtin_elementwise_fma(ay, y, ax * x));
}

__device__ __forceinline__ float comp(const float4& v, int j) {
  return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w));
}

template <bool kNormals>
__global__ void __launch_bounds__(kCpThreads) closestPointsKernel(ClosestPointsArgs a) {
  constexpr int T = kNormals ? kCpTileNormals : kCpTile;
  constexpr int C = kNormals ? 6 : 3;
  constexpr int E = 3 * T / kCpThreads; // floats of one array (coordinates or normals) a thread stages per tile
  static_assert(3 * T % kCpThreads == 0 && T % (4 * kCpWays) == 0, "a tile is whole passes of the workgroup and whole groups of four per wave");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* partD2 = smem + 2 * C * T;
  int32_t* partIndex = reinterpret_cast<int32_t*>(partD2 + kCpWays * kCpWaveSources);

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int b = int(blockIdx.x) / a.groups, g = int(blockIdx.x) % a.groups;
  const int N = a.N, M = a.M;
  const float kNaN = __builtin_nanf("");
  const float kInf = __builtin_inff();

  // ---- this lane's sources
  const int sBase = g * kCpWaveSources;
  const float* srcB = a.source + size_t(b) * size_t(N) * 3;
  float sx[kCpBlock], sy[kCpBlock], sz[kCpBlock], snx[kCpBlock], sny[kCpBlock], snz[kCpBlock], best[kCpBlock];
  int32_t bestIndex[kCpBlock];
#pragma unroll
  for (int r = 0; r < kCpBlock; ++r) {
    const int s = sBase + 64 * r + lane;
    const bool in = s < N;
    const size_t o = in ? size_t(s) * 3 : 0;
    sx[r] = in ? srcB[o] : kNaN, sy[r] = in ? srcB[o + 1] : kNaN, sz[r] = in ? srcB[o + 2] : kNaN;
    if constexpr (kNormals) {
      const float* nB = a.sourceNormals + size_t(b) * size_t(N) * 3;
      snx[r] = in ? nB[o] : kNaN, sny[r] = in ? nB[o + 1] : kNaN, snz[r] = in ? nB[o + 2] : kNaN;
    } else {
      snx[r] = sny[r] = snz[r] = 0.f;
    }
    best[r] = kInf, bestIndex[r] = -1;
  }

  // ---- the targets, tile by tile
  const float* tgtB = a.target + size_t(b) * a.targetStride;
  const float* tnB = kNormals ? a.targetNormals + size_t(b) * a.targetStride : nullptr;
  float stage[kNormals ? 2 * E : E];
  auto loadTile = [&](int t0) { // global -> registers; past the cloud's end: NaN coordinates, zero normals
    const int count = 3 * min(T, M - t0);
    const size_t base = size_t(t0) * 3;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int e = tid + kCpThreads * k;
      stage[k] = e < count ? tgtB[base + size_t(e)] : kNaN;
      if constexpr (kNormals) {
        stage[E + k] = e < count ? tnB[base + size_t(e)] : 0.f;
      }
    }
  };
  auto storeTile = [&](float* buf) { // registers -> LDS, [M][3] -> structure of arrays
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int e = tid + kCpThreads * k;
      const int t = e / 3, c = e - 3 * t;
      buf[c * T + t] = stage[k];
      if constexpr (kNormals) {
        buf[(3 + c) * T + t] = stage[E + k];
      }
    }
  };
  const int numTiles = (M + T - 1) / T;
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
    const int count = (min(T, M - t0) + 3) & ~3;
    const int lo = wave * (T / kCpWays);
    const int hi = min(lo + T / kCpWays, count);
#pragma unroll 1
    for (int t = lo; t < hi; t += 4) {
      const float4 tx = *reinterpret_cast<const float4*>(buf + t);
      const float4 ty = *reinterpret_cast<const float4*>(buf + T + t);
      const float4 tz = *reinterpret_cast<const float4*>(buf + 2 * T + t);
      float4 nx, ny, nz;
      if constexpr (kNormals) {
        nx = *reinterpret_cast<const float4*>(buf + 3 * T + t);
        ny = *reinterpret_cast<const float4*>(buf + 4 * T + t);
        nz = *reinterpret_cast<const float4*>(buf + 5 * T + t);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int32_t ti = t0 + t + j;
#pragma unroll
        for (int r = 0; r < kCpBlock; r += 2) {
          const float2v d2 = pairDist2(
              float2v{sx[r], sx[r + 1]}, float2v{sy[r], sy[r + 1]}, float2v{sz[r], sz[r + 1]}, comp(tx, j), comp(ty, j), comp(tz, j));
          bool take0 = d2.x < best[r], take1 = d2.y < best[r + 1]; // ordered: false for NaN, and for +inf against the initial +inf
          if constexpr (kNormals) {
            const float2v dot = pairDot(
                float2v{snx[r], snx[r + 1]}, float2v{sny[r], sny[r + 1]}, float2v{snz[r], snz[r + 1]}, comp(nx, j), comp(ny, j), comp(nz, j));
            take0 = take0 && dot.x >= a.minNormalDot, take1 = take1 && dot.y >= a.minNormalDot;
          }
          best[r] = take0 ? d2.x : best[r], best[r + 1] = take1 ? d2.y : best[r + 1];
          bestIndex[r] = take0 ? ti : bestIndex[r], bestIndex[r + 1] = take1 ? ti : bestIndex[r + 1];
        }
      }
    }
    if (more) {
      storeTile(smem + ((tile + 1) & 1) * C * T);
    }
    __syncthreads();
  }

  // ---- results: max_dist once, then every entry of every output
  auto write = [&](int s, float d2, int32_t i) {
    const bool valid = i >= 0 && d2 <= a.maxDist2;
    const size_t o = size_t(b) * size_t(N) + size_t(s);
    a.index[o] = valid ? i : -1;
    if (a.dist2 != nullptr) {
      a.dist2[o] = valid ? d2 : kInf;
    }
    if (a.points != nullptr) {
      const float* p = tgtB + (valid ? size_t(i) * 3 : 0);
      const float px = p[0], py = p[1], pz = p[2]; // (target 0 exists: M >= 1)
      a.points[3 * o] = valid ? px : 0.f, a.points[3 * o + 1] = valid ? py : 0.f, a.points[3 * o + 2] = valid ? pz : 0.f;
    }
  };
#pragma unroll
  for (int r = 0; r < kCpBlock; ++r) {
    partD2[wave * kCpWaveSources + 64 * r + lane] = best[r];
    partIndex[wave * kCpWaveSources + 64 * r + lane] = bestIndex[r];
  }
  __syncthreads();
#pragma unroll
  for (int local = tid; local < kCpWaveSources; local += kCpThreads) { // (one source per thread with a block of four)
    const int s = sBase + local;
    if (s < N) {
      float d2 = partD2[local];
      int32_t i = partIndex[local];
#pragma unroll
      for (int w = 1; w < kCpWays; ++w) {
        const float dw = partD2[w * kCpWaveSources + local];
        const int32_t iw = partIndex[w * kCpWaveSources + local];
        const bool take = iw >= 0 && (dw < d2 || (dw == d2 && iw < i)); // (d2 == +inf only with i == -1, and then dw < d2)
        d2 = take ? dw : d2, i = take ? iw : i;
      }
      write(s, d2, i);
    }
  }
}
static_assert(kCpBlock % 2 == 0 && kCpWaveSources % kCpThreads == 0, "sources go two at a time; the last step finishes whole passes of the workgroup");

size_t closestPointsLdsBytes(bool normals) {
  const size_t tile = size_t(normals ? 6 * kCpTileNormals : 3 * kCpTile);
  return (2 * tile + 2 * size_t(kCpWays) * kCpWaveSources) * sizeof(float);
}

// the checks every entry point makes before anything is touched; null = fine
const char* closestPointsRefusal(
    int32_t batch, int32_t N, int32_t M, const void* source, const void* target, const void* sn, const void* tn, float maxDist, float minDot,
    const void* index, ClosestPointsPlan* plan) {
  if (source == nullptr || target == nullptr || index == nullptr) {
    return "source / target / index is null";
  }
  if (batch < 1 || N < 1 || M < 1) {
    return "batch, num_source and num_target must be >= 1";
  }
  if (!(maxDist >= 0.f)) {
    return "max_dist must be >= 0 (+inf allowed), not negative or NaN";
  }
  if ((sn == nullptr) != (tn == nullptr)) {
    return "source_normals and target_normals: both or neither";
  }
  if (sn != nullptr && std::isnan(minDot)) {
    return "min_normal_dot is NaN";
  }
  if (!closestPointsPlan(batch, N, M, sn != nullptr, plan)) {
    return "the launch grid exceeds 2^31 - 1 workgroups";
  }
  return nullptr;
}

} // namespace
} // namespace mmx

extern "C" {

int32_t mmx_closest_points_plan(
    int32_t batch, int32_t num_source, int32_t num_target, int32_t with_normals, int32_t* sources_per_workgroup, int32_t* target_tile,
    int32_t* target_ways) {
  mmx::ClosestPointsPlan p;
  if (!mmx::closestPointsPlan(batch, num_source, num_target, with_normals != 0, &p)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, "mmx_closest_points_plan: a size below 1, or a launch grid beyond 2^31 - 1 workgroups");
  }
  if (sources_per_workgroup != nullptr) {
    *sources_per_workgroup = p.sourcesPerWorkgroup;
  }
  if (target_tile != nullptr) {
    *target_tile = p.targetTile;
  }
  if (target_ways != nullptr) {
    *target_ways = p.targetWays;
  }
  return MMX_OK;
}

int32_t mmx_closest_points(
    int32_t batch,
    int32_t num_source,
    int32_t num_target,
    const float* source_dev,
    const float* target_dev,
    int32_t target_shared,
    const float* source_normals_dev,
    const float* target_normals_dev,
    float max_dist,
    float min_normal_dot,
    int32_t* index_dev,
    float* dist2_dev,
    float* points_dev,
    void* stream) {
  mmx::ClosestPointsPlan plan;
  if (const char* why = mmx::closestPointsRefusal(
          batch, num_source, num_target, source_dev, target_dev, source_normals_dev, target_normals_dev, max_dist, min_normal_dot, index_dev, &plan)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string("mmx_closest_points: ") + why);
  }
  const bool normals = source_normals_dev != nullptr;
  mmx::ClosestPointsArgs a{};
  a.N = num_source, a.M = num_target, a.groups = int32_t(plan.workgroups / batch);
  a.source = source_dev, a.target = target_dev, a.sourceNormals = source_normals_dev, a.targetNormals = target_normals_dev;
  a.targetStride = target_shared != 0 ? 0 : size_t(num_target) * 3;
  a.maxDist2 = max_dist * max_dist; // (float32: +inf stays +inf)
  a.minNormalDot = min_normal_dot;
  a.index = index_dev, a.dist2 = dist2_dev, a.points = points_dev;
  const dim3 grid(unsigned(plan.workgroups)), block(mmx::kCpThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (normals) {
    hipLaunchKernelGGL(mmx::closestPointsKernel<true>, grid, block, mmx::closestPointsLdsBytes(true), s, a);
  } else {
    hipLaunchKernelGGL(mmx::closestPointsKernel<false>, grid, block, mmx::closestPointsLdsBytes(false), s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    return mmx::failWith(MMX_ERR_DEVICE, std::string("mmx_closest_points: ") + hipGetErrorString(e));
  }
  return MMX_OK;
}

int32_t mmx_closest_points_host(
    int32_t batch,
    int32_t num_source,
    int32_t num_target,
    const float* source_host,
    const float* target_host,
    int32_t target_shared,
    const float* source_normals_host,
    const float* target_normals_host,
    float max_dist,
    float min_normal_dot,
    int32_t* index_host,
    float* dist2_host,
    float* points_host) {
  mmx::ClosestPointsPlan plan;
  if (const char* why = mmx::closestPointsRefusal(
          batch, num_source, num_target, source_host, target_host, source_normals_host, target_normals_host, max_dist, min_normal_dot, index_host,
          &plan)) {
    return mmx::failWith(MMX_ERR_INVALID_ARGUMENT, std::string("mmx_closest_points_host: ") + why);
  }
  const size_t nSrc = size_t(batch) * size_t(num_source), nTgt = (target_shared != 0 ? size_t(1) : size_t(batch)) * size_t(num_target);
  const bool normals = source_normals_host != nullptr;
  struct Buf { // (freed on every way out)
    void* p = nullptr;
    ~Buf() {
      if (p != nullptr) {
        (void)hipFree(p);
      }
    }
  } src, tgt, sn, tn, idx, d2, pts;
  auto fail = [](hipError_t e, const char* what) {
    return mmx::failWith(e == hipErrorOutOfMemory ? MMX_ERR_OUT_OF_MEMORY : MMX_ERR_DEVICE, std::string("mmx_closest_points_host: ") + what + ": " + hipGetErrorString(e));
  };
  auto up = [&](Buf& buf, const void* host, size_t bytes) {
    hipError_t e = hipMalloc(&buf.p, bytes);
    if (e == hipSuccess && host != nullptr) {
      e = hipMemcpy(buf.p, host, bytes, hipMemcpyHostToDevice);
    }
    return e;
  };
  hipError_t e = up(src, source_host, nSrc * 3 * sizeof(float));
  e = e != hipSuccess ? e : up(tgt, target_host, nTgt * 3 * sizeof(float));
  if (normals) {
    e = e != hipSuccess ? e : up(sn, source_normals_host, nSrc * 3 * sizeof(float));
    e = e != hipSuccess ? e : up(tn, target_normals_host, nTgt * 3 * sizeof(float));
  }
  e = e != hipSuccess ? e : up(idx, nullptr, nSrc * sizeof(int32_t));
  if (dist2_host != nullptr) {
    e = e != hipSuccess ? e : up(d2, nullptr, nSrc * sizeof(float));
  }
  if (points_host != nullptr) {
    e = e != hipSuccess ? e : up(pts, nullptr, nSrc * 3 * sizeof(float));
  }
  if (e != hipSuccess) {
    return fail(e, "upload");
  }
  const int32_t rc = mmx_closest_points(
      batch, num_source, num_target, static_cast<const float*>(src.p), static_cast<const float*>(tgt.p), target_shared,
      static_cast<const float*>(sn.p), static_cast<const float*>(tn.p), max_dist, min_normal_dot, static_cast<int32_t*>(idx.p),
      static_cast<float*>(d2.p), static_cast<float*>(pts.p), nullptr);
  if (rc != MMX_OK) {
    return rc;
  }
  e = hipDeviceSynchronize();
  e = e != hipSuccess ? e : hipMemcpy(index_host, idx.p, nSrc * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (dist2_host != nullptr) {
    e = e != hipSuccess ? e : hipMemcpy(dist2_host, d2.p, nSrc * sizeof(float), hipMemcpyDeviceToHost);
  }
  if (points_host != nullptr) {
    e = e != hipSuccess ? e : hipMemcpy(points_host, pts.p, nSrc * 3 * sizeof(float), hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    return fail(e, "download");
  }
  return MMX_OK;
}

} // extern "C"
