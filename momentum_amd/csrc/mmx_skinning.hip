// mmx_skinning.hip -- linear-blend skinning, skeleton state -> posed vertices, forward and backward (gfx950 / CDNA4, wave64).
// The counterpart of pymomentum/backend/triton_skinning.py (_forward_kernel / _backward_kernel) and momentum's applySSD.
//
//   out[b][v] = sum_k weight[v][k] ( t_j + s_j qrot(q_j, p_vk) ),   p_vk = A_j rest_v + a_j,   j = joint[v][k]
//
// with (t_j, q_j, s_j) the state row [b][j] and [A_j | a_j] the joint's inverse bind.  qrot is the polynomial of
// mmx_device.hpp, p + 2 w (u x p) + 2 u x (u x p): linear in p, so t + s qrot(q, .) is the affine map [s R(q) | t] with
// R(q) = (1 - 2 |u|^2) I + 2 u u^T + 2 w [u]x (qmatCol) for ANY q -- the quaternion is used as the state holds it.
//
// skinPointsKernel<false>  forward.  A 256-thread workgroup takes a tile of 1024 vertices of one instance.  It first builds
//     the posed affine of every joint, M_j = [s R A_j | s R a_j + t] (12 floats, computed in double and rounded once), in LDS;
//     then a thread takes four vertices 256 apart: K index and weight loads (shared by the batch, L2-resident), K reads of
//     M_j (three ds_read_b128), one 12-byte streaming store -- a wave's stores cover 768 contiguous bytes.  A zero-weight
//     slot is skipped, so a non-finite state row behind padding contributes nothing.
// skinPointsKernel<true>   the rest gradient, rest_grad[b][v] = sum_k w (s R A_j)^T g[b][v]: the same kernel with the
//     cotangent in the place of the rest position and the 3 x 3 part of M_j applied transposed.  No reduction.
// skinPointsBackwardKernel the state gradient.  A joint's twelve sums over its influences,
//         F_j = sum w g   (3)        N_j = sum w g p_vk^T   (9)
//     are produced by ONE wavefront: its lanes stride through the joint's entries of the joint-sorted influence list
//     (mmx_skin_tables.hpp: sorted by (joint, vertex, slot)), gather g[b][v] and the rest position, recompute p_vk and
//     accumulate in double; a fixed cross-lane tree (four DPP steps in a row of sixteen, then the four rows) follows and the
//     eight channels come from the sums in double:
//         g_t = F    g_s = phi(q)    g_q = s dphi/dq,    phi(q) = <R(q), N> = (1 - 2 |u|^2) tr N + 2 u^T N u + 2 w u . ax(N)
//         dphi/du = -4 tr N u + 2 (N + N^T) u + 2 w ax(N)    dphi/dw = 2 u . ax(N)    ax(N) = (N21 - N12, N02 - N20, N10 - N01)
//     -- the exact derivative of the polynomial, no renormalisation term.  A joint without an entry gets eight exact zeros.
//     Waves take contiguous joint ranges from a host-built partition balanced by entry count (SkinTables::waveStart); a
//     joint's order of summation is lane = entry mod 64, then the tree: it depends on its own entry list only.
// No atomics, no scratch; no instance reads another's data.  The backward kernel uses no LDS.
//
// LDS map of skinPointsKernel (floats): M [J][12]
#include "mmx_device.hpp"
#include "mmx_kernels.hpp"

namespace mmx {

constexpr int kSkinThreads = 256, kSkinPerThread = 4;
static_assert(kSkinThreads * kSkinPerThread == kSkinTile, "a tile is four passes of the workgroup");

template <bool kRestGrad>
__global__ void __launch_bounds__(kSkinThreads) skinPointsKernel(
    SkinDev sk,
    int tiles,
    const float* __restrict__ state, // [B][J][8]
    const float* __restrict__ in, // forward: rest positions [V][3] or [B][V][3]; rest gradient: dL/dout [B][V][3]
    size_t inStride, // floats between two instances of `in` (0: shared)
    float* __restrict__ out) { // [B][V][3] every entry written
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int b = int(blockIdx.x) / tiles, tile = int(blockIdx.x) % tiles;
  const int J = sk.J, V = sk.V, K = sk.K;
  // ---- the posed affines: one row of one joint per thread, in double, rounded once
  for (int i = tid; i < 3 * J; i += kSkinThreads) {
    const int j = i / 3, r = i - 3 * j;
    const float* w = state + (size_t(b) * size_t(J) + size_t(j)) * 8;
    const float* ib = sk.inverseBind + size_t(j) * 12;
    const double s = double(w[7]);
    const DQ q{double(w[3]), double(w[4]), double(w[5]), double(w[6])};
    const D3 c0 = qmatCol(q, 0), c1 = qmatCol(q, 1), c2 = qmatCol(q, 2);
    auto pick = [r](const D3& c) { return r == 0 ? c.x : (r == 1 ? c.y : c.z); };
    const double sx = s * pick(c0), sy = s * pick(c1), sz = s * pick(c2); // row r of s R
    double m[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      m[c] = sx * double(ib[c]) + sy * double(ib[4 + c]) + sz * double(ib[8 + c]);
    }
    reinterpret_cast<float4*>(smem)[i] = make_float4(float(m[0]), float(m[1]), float(m[2]), float(m[3] + double(w[r])));
  }
  __syncthreads();
  // ---- one vertex per lane, four passes.  Every load of a pass is issued before the first use: the K weights and joint
  // indices without a branch (k < K is uniform), then the LDS reads of all slots; a zero-weight slot is dropped by a select
  const float* inB = in + size_t(b) * inStride;
  float* outB = out + size_t(b) * size_t(V) * 3;
#pragma unroll 1
  for (int i = 0; i < kSkinPerThread; ++i) {
    const int v = tile * kSkinTile + i * kSkinThreads + tid;
    if (v >= V) {
      break;
    }
    const float x = inB[size_t(v) * 3], y = inB[size_t(v) * 3 + 1], z = inB[size_t(v) * 3 + 2];
    const int32_t* jv = sk.joint + size_t(v) * size_t(K);
    const float* wv = sk.weight + size_t(v) * size_t(K);
    float wk[MMX_MAX_SKIN_INFLUENCES];
    int jk[MMX_MAX_SKIN_INFLUENCES];
#pragma unroll
    for (int k = 0; k < MMX_MAX_SKIN_INFLUENCES; ++k) {
      wk[k] = k < K ? wv[k] : 0.f;
      jk[k] = k < K ? jv[k] : 0;
    }
    float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
    for (int k = 0; k < MMX_MAX_SKIN_INFLUENCES; ++k) {
      if (k < K) {
        const float4* M = reinterpret_cast<const float4*>(smem) + 3 * jk[k];
        const float4 r0 = M[0], r1 = M[1], r2 = M[2];
        float px, py, pz;
        if constexpr (kRestGrad) {
          px = r0.x * x + r1.x * y + r2.x * z, py = r0.y * x + r1.y * y + r2.y * z, pz = r0.z * x + r1.z * y + r2.z * z;
        } else {
          px = r0.x * x + r0.y * y + r0.z * z + r0.w, py = r1.x * x + r1.y * y + r1.z * z + r1.w, pz = r2.x * x + r2.y * y + r2.z * z + r2.w;
        }
        const bool on = wk[k] != 0.f; // (padding: its joint's state may be anything)
        ax += on ? wk[k] * px : 0.f, ay += on ? wk[k] * py : 0.f, az += on ? wk[k] * pz : 0.f;
      }
    }
    float* o = outB + size_t(v) * 3;
    __builtin_nontemporal_store(ax, o);
    __builtin_nontemporal_store(ay, o + 1);
    __builtin_nontemporal_store(az, o + 2);
  }
}

__global__ void __launch_bounds__(kSkinThreads) skinPointsBackwardKernel(
    SkinDev sk,
    int groups,
    const float* __restrict__ state, // [B][J][8]
    const float* __restrict__ rest, // [V][3] or [B][V][3]
    size_t restStride, // floats between two instances of `rest` (0: shared)
    const float* __restrict__ outGrad, // [B][V][3]
    float* __restrict__ stateGrad) { // [B][J][8] every entry written
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int b = int(blockIdx.x) / groups;
  const int gw = (int(blockIdx.x) % groups) * (kSkinThreads / 64) + wave;
  if (gw >= sk.numWaves) {
    return;
  }
  const int J = sk.J;
  const float* g = outGrad + size_t(b) * size_t(sk.V) * 3;
  const float* rv = rest + size_t(b) * restStride;
  const int j1 = sk.waveStart[gw + 1];
#pragma unroll 1
  for (int j = sk.waveStart[gw]; j < j1; ++j) {
    const int e0 = sk.jointStart[j], e1 = sk.jointStart[j + 1];
    float* o = stateGrad + (size_t(b) * size_t(J) + size_t(j)) * 8;
    if (e0 == e1) { // no influence: exact zeros, whatever the state row holds
      if (lane < 8) {
        o[lane] = 0.f;
      }
      continue;
    }
    const float* ib = sk.inverseBind + size_t(j) * 12;
    const double a00 = ib[0], a01 = ib[1], a02 = ib[2], a03 = ib[3];
    const double a10 = ib[4], a11 = ib[5], a12 = ib[6], a13 = ib[7];
    const double a20 = ib[8], a21 = ib[9], a22 = ib[10], a23 = ib[11];
    double fx = 0.0, fy = 0.0, fz = 0.0;
    double n00 = 0.0, n01 = 0.0, n02 = 0.0, n10 = 0.0, n11 = 0.0, n12 = 0.0, n20 = 0.0, n21 = 0.0, n22 = 0.0;
    // four strides of 64 entries per trip, every load of a trip issued before its first use; a lane takes its entries in
    // ascending order whatever the grouping, and a slot past the end adds an exact zero
#pragma unroll 1
    for (int base = e0 + lane; base < e1 + lane; base += 4 * 64) {
      size_t v3[4];
      double wt[4], gx[4], gy[4], gz[4], rx[4], ry[4], rz[4];
      bool on[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = base + 64 * i;
        on[i] = e < e1;
        v3[i] = on[i] ? size_t(sk.entryVertex[e]) * 3 : 0;
        wt[i] = on[i] ? double(sk.entryWeight[e]) : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gx[i] = double(g[v3[i]]), gy[i] = double(g[v3[i] + 1]), gz[i] = double(g[v3[i] + 2]);
        rx[i] = double(rv[v3[i]]), ry[i] = double(rv[v3[i] + 1]), rz[i] = double(rv[v3[i] + 2]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double wx = on[i] ? wt[i] * gx[i] : 0.0, wy = on[i] ? wt[i] * gy[i] : 0.0, wz = on[i] ? wt[i] * gz[i] : 0.0;
        const double px = a00 * rx[i] + a01 * ry[i] + a02 * rz[i] + a03;
        const double py = a10 * rx[i] + a11 * ry[i] + a12 * rz[i] + a13;
        const double pz = a20 * rx[i] + a21 * ry[i] + a22 * rz[i] + a23;
        fx += wx, fy += wy, fz += wz;
        n00 += wx * px, n01 += wx * py, n02 += wx * pz;
        n10 += wy * px, n11 += wy * py, n12 += wy * pz;
        n20 += wz * px, n21 += wz * py, n22 += wz * pz;
      }
    }
    fx = waveReduceSum(fx), fy = waveReduceSum(fy), fz = waveReduceSum(fz);
    n00 = waveReduceSum(n00), n01 = waveReduceSum(n01), n02 = waveReduceSum(n02);
    n10 = waveReduceSum(n10), n11 = waveReduceSum(n11), n12 = waveReduceSum(n12);
    n20 = waveReduceSum(n20), n21 = waveReduceSum(n21), n22 = waveReduceSum(n22);
    // ---- the eight channels from (F, N, q, s)
    const float* w = state + (size_t(b) * size_t(J) + size_t(j)) * 8;
    const double ux = w[3], uy = w[4], uz = w[5], qw = w[6], s = w[7];
    const double tr = n00 + n11 + n22;
    const double axx = n21 - n12, axy = n02 - n20, axz = n10 - n01;
    const double nux = n00 * ux + n01 * uy + n02 * uz, nuy = n10 * ux + n11 * uy + n12 * uz, nuz = n20 * ux + n21 * uy + n22 * uz; // N u
    const double ntx = n00 * ux + n10 * uy + n20 * uz, nty = n01 * ux + n11 * uy + n21 * uz, ntz = n02 * ux + n12 * uy + n22 * uz; // N^T u
    const double uu = ux * ux + uy * uy + uz * uz, uax = ux * axx + uy * axy + uz * axz;
    const double phi = (1.0 - 2.0 * uu) * tr + 2.0 * (ux * nux + uy * nuy + uz * nuz) + 2.0 * qw * uax;
    const double dx = s * (-4.0 * tr * ux + 2.0 * (nux + ntx) + 2.0 * qw * axx);
    const double dy = s * (-4.0 * tr * uy + 2.0 * (nuy + nty) + 2.0 * qw * axy);
    const double dz = s * (-4.0 * tr * uz + 2.0 * (nuz + ntz) + 2.0 * qw * axz);
    const double dw = s * (2.0 * uax);
    if (lane < 8) { // one 32-byte store of the row
      const double c = lane == 0 ? fx : lane == 1 ? fy : lane == 2 ? fz : lane == 3 ? dx : lane == 4 ? dy : lane == 5 ? dz : lane == 6 ? dw : phi;
      o[lane] = float(c);
    }
  }
}

namespace {
bool skinGrid(int B, int perInstance, unsigned* grid) {
  const long long n = (long long)B * perInstance;
  if (B <= 0 || perInstance <= 0 || n > 0x7fffffffLL) {
    return false;
  }
  *grid = unsigned(n);
  return true;
}

template <bool kRestGrad>
hipError_t launchSkinForward(const SkinDev& sk, int B, const float* state, const float* in, size_t inStride, float* out, hipStream_t stream) {
  const size_t lds = size_t(sk.J) * 12 * sizeof(float);
  const int tiles = (sk.V + kSkinTile - 1) / kSkinTile;
  unsigned grid = 0;
  if (lds > 160 * 1024 - 64 || !skinGrid(B, tiles, &grid)) {
    return hipErrorInvalidValue;
  }
  static LdsLimitCache ldsLimit; // (one per instantiation)
  hipError_t rc = ldsLimit.ensure(reinterpret_cast<const void*>(skinPointsKernel<kRestGrad>), lds);
  if (rc != hipSuccess) {
    return rc;
  }
  hipLaunchKernelGGL(skinPointsKernel<kRestGrad>, dim3(grid), dim3(kSkinThreads), lds, stream, sk, tiles, state, in, inStride, out);
  return hipGetLastError();
}
} // namespace

hipError_t launchSkinPoints(const SkinDev& sk, int B, const float* state, const float* restInst, float* out, hipStream_t stream) {
  const bool inst = restInst != nullptr;
  return launchSkinForward<false>(sk, B, state, inst ? restInst : sk.rest, inst ? size_t(sk.V) * 3 : 0, out, stream);
}

hipError_t launchSkinRestGrad(const SkinDev& sk, int B, const float* state, const float* outGrad, float* restGrad, hipStream_t stream) {
  return launchSkinForward<true>(sk, B, state, outGrad, size_t(sk.V) * 3, restGrad, stream);
}

hipError_t launchSkinPointsBackward(
    const SkinDev& sk, int B, const float* state, const float* restInst, const float* outGrad, float* stateGrad, hipStream_t stream) {
  const int groups = (sk.numWaves + kSkinThreads / 64 - 1) / (kSkinThreads / 64);
  unsigned grid = 0;
  if (!skinGrid(B, groups, &grid)) {
    return hipErrorInvalidValue;
  }
  const bool inst = restInst != nullptr;
  hipLaunchKernelGGL(
      skinPointsBackwardKernel, dim3(grid), dim3(kSkinThreads), 0, stream, sk, groups, state, inst ? restInst : sk.rest,
      inst ? size_t(sk.V) * 3 : 0, outGrad, stateGrad);
  return hipGetLastError();
}

} // namespace mmx
