// mmx_skin_normal_equations.hip -- mmx_skin_normal_equations: H = J^T J, g = J^T (sigma f) and the error of a batch of
// vertex constraints on a skinned mesh, over the problem's enabled parameters (gfx950 / CDNA4, wave64).  The Gauss-Newton
// terms of momentum's vertex error function (position and plane types) in the layout of mmx_eval_normal_equations.
//
//   x_c = sum_{i<S} beta_ci out[b][v_ci],   out = mmx_skin_points on the skeleton state at theta
//   MMX_VC_POSITION  f = x_c - target_c (three rows)        MMX_VC_PLANE  f = n_c . (x_c - target_c) (one row)
//   sigma_c = sqrt(fw w_c),   H = sum rows (sigma df/dtheta)^T (sigma df/dtheta),   g = sum rows (sigma df/dtheta)^T sigma f
//
// Every influence (joint j, coefficient beta w, posed point y = t_j + s_j R_j p) of a constraint moves rigidly with j, so a
// source (joint a, dof) of a column sees the constraint through two sums over the influences whose joint lies under a
// (DFS interval): m0 = sum coef and m1 = sum coef y.  With d = m1 - m0 t_a the point's derivative is sourceDerivative's
// (mmx_device.hpp): translation m0 x the parent's linear column, rotation axis x d, scale ln 2 d -- which is what
// skeleton_state_backward(skin_points_backward(.)) returns for the row's cotangent (N_sub - t_a x F_sub = sum coef (y - t_a) x g).
//
// One 256-thread workgroup per instance:
//   setup   theta -> LDS; blockFk<.., kUnitLocal> (the state backward's forward: local quaternions renormalised in double),
//           the posed affines M_j as skinPointsKernel builds them, per source of an enabled column (t_a, axis / linear column)
//   per tile of 32 residual rows
//     S1    one thread per (constraint, corner): the K influences -> (DFS position, beta w, y) in LDS, beta out[v]
//     S2    one thread per row: x_c, f, sigma; sigma f, sigma n; the row's share of the error in double (kept by the thread)
//     T     one thread per (constraint, column): m0, m1 per source, the point's derivative D; the rows' entries sigma D_k or
//           sigma n . D into the [32 x nPad] tile (row-major: the 32 lanes of a half-wave read 32 consecutive floats -- no
//           bank conflict for ds_read_b32 whatever the row stride).  A skipped constraint's rows are exact zeros.
//     H     tile^T tile on the matrix cores, v_mfma_f32_32x32x2_f32: 16 steps per 32 x 32 block of H, the lower block
//           triangle dealt to the four waves (block I (I + 1) / 2 + Jb to wave index mod 4), accumulators in registers
//           across all tiles; g by 256 threads (column, half of the rows) in double, fixed order
//   store   the blocks and their mirrors (H exactly symmetric: a diagonal block's (i, j) and (j, i) are the same products
//           in the same order), g = half 0 + half 1, err = the 32 row threads' sums in row order
// No atomics, no scratch, no instance reads another's data; tile composition depends on (C, S, type) only.
//
// LDS map (floats; every piece rounded up to a multiple of 4):
//   th [P] | js [kJs J] | fkA [fkBufFloats(J)] | R = max(fkBufFloats(J), 2 x 7 J) | M [12 J] | tin [J] | colRange [2 n]
//   | src [kSrcRec nsrc] | tile [32 nPad] | infTin [32 S K] | infCoef [32 S K] | infY [3 x 32 S K] | cOut [3 x 32 S]
//   | cAct [32] | rowRes [32] | rowSig [32] | rowN [96] | red (double) [2 x 128 + 32]
#include "mmx_device.hpp"
#include "mmx_fused_helpers.hpp"
#include "mmx_kernels.hpp"
#include "mmx_skin_normal_equations_plan.hpp"
#include "mmx_tree.hpp"

namespace mmx {

namespace {

typedef float sne32x16 __attribute__((ext_vector_type(16)));

constexpr int kSneThreads = 256, kSneTileRows = 32, kSneMaxBlocksPerWave = 3;
constexpr int kSrcRec = 11; // tin, tout, dof, weight, t_a (3), axis or linear column (3), pad (odd stride: lanes = columns)
static_assert(kSkinNeMaxSolved == 128, "four 32-wide block columns: ten lower blocks, at most three per wave");

struct SkinNeLds {
  float *th, *js, *jd, *M, *src, *tile, *infCoef, *infY, *cOut, *rowRes, *rowSig, *rowN;
  double *fkA, *fkB, *red;
  int *tin, *colRange, *infTin, *cAct;
};

} // namespace

__host__ __device__ inline size_t skinNeLdsFloats(int J, int P, int n, int nsrc, int S, int K, SkinNeLds* out, float* base) {
  size_t off = 0;
  auto take = [&](size_t count) {
    const size_t o = off;
    off += alignUp4(count);
    return o;
  };
  const int nPad = (n + 31) & ~31, inf = kSneTileRows * S * K;
  const size_t oTh = take(P), oJs = take(size_t(kJs) * J), oFk = take(fkBufFloats(J));
  const size_t own = alignUp4(size_t(kC1) * J);
  const size_t oR = take(fkBufFloats(J) > 2 * own ? fkBufFloats(J) : 2 * own);
  const size_t oM = take(size_t(12) * J), oTin = take(J), oCol = take(size_t(2) * n), oSrc = take(size_t(kSrcRec) * nsrc);
  const size_t oTile = take(size_t(kSneTileRows) * nPad), oIt = take(inf), oIc = take(inf), oIy = take(size_t(3) * inf);
  const size_t oOut = take(size_t(3) * kSneTileRows * S), oAct = take(kSneTileRows), oRes = take(kSneTileRows), oSig = take(kSneTileRows);
  const size_t oN = take(3 * kSneTileRows), oRed = take(2 * (2 * size_t(kSkinNeMaxSolved) + kSneTileRows));
  if (out != nullptr) {
    out->th = base + oTh, out->js = base + oJs, out->jd = base + oR, out->M = base + oM, out->src = base + oSrc;
    out->tile = base + oTile, out->infCoef = base + oIc, out->infY = base + oIy, out->cOut = base + oOut;
    out->rowRes = base + oRes, out->rowSig = base + oSig, out->rowN = base + oN;
    out->fkA = reinterpret_cast<double*>(base + oFk), out->fkB = reinterpret_cast<double*>(base + oR);
    out->red = reinterpret_cast<double*>(base + oRed);
    out->tin = reinterpret_cast<int*>(base + oTin), out->colRange = reinterpret_cast<int*>(base + oCol);
    out->infTin = reinterpret_cast<int*>(base + oIt), out->cAct = reinterpret_cast<int*>(base + oAct);
  }
  return off;
}

// kSplit = false: the kernel of the header, one workgroup per instance (sp is not read).  kSplit = true: workgroup blockIdx.x is part
// blockIdx.x % Pe of instance blockIdx.x / Pe; it repeats the set-up, runs the tile loop over its part's tiles
// (mmx_skin_normal_equations_plan.hpp) and stores its raw partial results to the workspace instead of H / g / err:
// the accumulators as the waves hold them ([block][reg][lane]: a wave's store of a register is 64 consecutive floats), per
// column the double h0 + h1, and the double sum of the 32 row threads' errors in row order.  Nothing of another part is read.
struct SkinNeSplitDev {
  SkinNeWorkspace ws; // ws.parts = Pe
  char* base; // the workspace
};

template <bool kSplit>
__global__ void __launch_bounds__(kSneThreads) skinNormalEquationsKernel(
    RigDev rig,
    SkinNeColumnsDev cols,
    SkinDev sk,
    VertexConstraintsDev vc,
    const float* __restrict__ theta, // [B][P]
    float* __restrict__ H, // [B][n][n] or null
    float* __restrict__ g, // [B][n] or null
    double* __restrict__ err, // [B] or null
    SkinNeSplitDev sp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int kT = kSneThreads;
  const int b = kSplit ? int(blockIdx.x) / sp.ws.parts : int(blockIdx.x), tid = threadIdx.x;
  const int part = kSplit ? int(blockIdx.x) - b * sp.ws.parts : 0;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  selectInstanceRig(rig, b);
  const int J = rig.J, P = rig.P, n = cols.n, nsrc = cols.nsrc;
  const int S = vc.S, K = sk.K, V = sk.V, C = vc.C;
  const int nPad = (n + 31) & ~31, nb = nPad >> 5, nInf = S * K;
  const bool plane = vc.type == MMX_VC_PLANE;
  SkinNeLds t;
  skinNeLdsFloats(J, P, n, nsrc, S, K, &t, smem);
  FusedLds s{};
  s.th = t.th, s.js = t.js, s.fkA = t.fkA, s.fkB = t.fkB, s.jd = t.jd;
  RigView rv;
  rv.J = J, rv.P = P, rv.R = rig.R, rv.numLevels = rig.numLevels, rv.jumpRounds = rig.jumpRounds;
  rv.parent = rig.parent, rv.preRot = rig.preRot, rv.offset = rig.offset;
  rv.ptOuter = rig.ptOuter, rv.ptInner = rig.ptInner, rv.ptValue = rig.ptValue, rv.ptOffsets = rig.ptOffsets;
  rv.hasOffsets = rig.ptOffsetsNonZero != 0;
  rv.levelOrder = rig.levelOrder, rv.levelStart = rig.levelStart;
  rv.rowRec = rig.ptRowRec, rv.numRowRec = rig.numRowRec;
  for (int i = tid; i < P; i += kT) {
    s.th[i] = theta[size_t(b) * P + i];
  }
  for (int i = tid; i < J; i += kT) {
    t.tin[i] = cols.jointTin[i];
  }
  for (int c = tid; c < n; c += kT) {
    const int p = cols.enabledList[c];
    t.colRange[2 * c] = cols.colStart[p];
    t.colRange[2 * c + 1] = cols.colStart[p + 1];
  }
  __syncthreads();
  // ---- forward kinematics with the rotation axes, local quaternions renormalised in double (ends with a barrier)
  blockFk<true, kT, true>(rv, s, s.th, tid, true);
  // ---- the posed affines (skinPointsKernel's: one row of one joint per thread, in double, rounded once)
  for (int i = tid; i < 3 * J; i += kT) {
    const int j = i / 3, r = i - 3 * j;
    const float* w = s.js + kJs * j;
    const float* ib = sk.inverseBind + size_t(j) * 12;
    const double sc = double(w[7]);
    const DQ q{double(w[3]), double(w[4]), double(w[5]), double(w[6])};
    const D3 c0 = qmatCol(q, 0), c1 = qmatCol(q, 1), c2 = qmatCol(q, 2);
    auto pick = [r](const D3& c) { return r == 0 ? c.x : (r == 1 ? c.y : c.z); };
    const double sx = sc * pick(c0), sy = sc * pick(c1), sz = sc * pick(c2);
    double m[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      m[c] = sx * double(ib[c]) + sy * double(ib[4 + c]) + sz * double(ib[8 + c]);
    }
    reinterpret_cast<float4*>(t.M)[i] = make_float4(float(m[0]), float(m[1]), float(m[2]), float(m[3] + double(w[r])));
  }
  // ---- per source of an enabled column: interval, dof, weight, t_a and the axis (rotation) or linear column (translation)
  for (int e = tid; e < nsrc; e += kT) {
    const ColumnSourceDev cs = cols.colSources[e];
    const float* a = s.js + kJs * cs.joint;
    F3 ax{0.f, 0.f, 0.f};
    if (cs.dof < 3) {
      ax = transAxisCol(s.js, cs.parent, cs.dof);
    } else if (cs.dof < 6) {
      const float* x = a + 8 + 3 * (cs.dof - 3);
      ax = F3{x[0], x[1], x[2]};
    }
    float* o = t.src + kSrcRec * e;
    o[0] = __int_as_float(cs.tin), o[1] = __int_as_float(cs.tout), o[2] = __int_as_float(cs.dof), o[3] = cs.weight;
    o[4] = a[0], o[5] = a[1], o[6] = a[2], o[7] = ax.x, o[8] = ax.y, o[9] = ax.z;
  }
  __syncthreads();

  const int rows = plane ? C : 3 * C, tiles = (rows + kSneTileRows - 1) / kSneTileRows;
  const size_t bC = size_t(b) * size_t(C);
  const int32_t* vB = vc.vertex != nullptr ? vc.vertex + bC * S : nullptr;
  const float* baryB = vc.bary != nullptr ? vc.bary + bC * S : nullptr;
  const float* tgtB = vc.target + bC * 3;
  const float* nrmB = vc.normal != nullptr ? vc.normal + bC * 3 : nullptr;
  const float* wB = vc.weight != nullptr ? vc.weight + bC : nullptr;
  const float* restB = vc.rest != nullptr ? vc.rest + size_t(b) * size_t(V) * 3 : sk.rest;
  // the wave's blocks of the lower block triangle
  const int numBlocks = nb * (nb + 1) / 2;
  int bI[kSneMaxBlocksPerWave], bJ[kSneMaxBlocksPerWave];
  sne32x16 acc[kSneMaxBlocksPerWave];
#pragma unroll
  for (int q = 0; q < kSneMaxBlocksPerWave; ++q) {
    const int idx = wave + 4 * q;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= idx) {
      ++I;
    }
    bI[q] = I, bJ[q] = idx - I * (I + 1) / 2;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[q][r] = 0.f;
    }
  }
  const int gCol = tid & (kSkinNeMaxSolved - 1), gHalf = tid >> 7;
  double gAcc = 0.0, errAcc = 0.0;

  const int tileBegin = kSplit ? skinNePartBegin(part, tiles, sp.ws.parts) : 0;
  const int tileEnd = kSplit ? skinNePartBegin(part + 1, tiles, sp.ws.parts) : tiles;
#pragma unroll 1
  for (int tile = tileBegin; tile < tileEnd; ++tile) {
    const int row0 = tile * kSneTileRows;
    const int rowEnd = min(rows, row0 + kSneTileRows); // one past the tile's last real row
    const int c0 = plane ? row0 : row0 / 3, c1 = plane ? rowEnd - 1 : (rowEnd - 1) / 3;
    const int nCons = c1 - c0 + 1; // <= 32
    // ---- S1: the influences of one corner of one constraint
    for (int it = tid; it < nCons * S; it += kT) {
      const int ci = it / S, sIdx = it - ci * S, c = c0 + ci;
      const float w = wB != nullptr ? wB[c] : 1.f;
      bool act = w > 0.f; // (false for a NaN)
      int v = 0;
      for (int q = 0; q < S; ++q) {
        const int vq = vB != nullptr ? vB[size_t(c) * S + q] : c;
        act = act && vq >= 0 && vq < V;
        v = q == sIdx ? vq : v;
      }
      int* iTin = t.infTin + ci * nInf + sIdx * K;
      float* iCoef = t.infCoef + ci * nInf + sIdx * K;
      float* iY = t.infY + 3 * (ci * nInf + sIdx * K);
      float ox = 0.f, oy = 0.f, oz = 0.f, beta = 1.f;
      if (act) { // (an index outside [0, V) is never dereferenced)
        beta = baryB != nullptr ? baryB[size_t(c) * S + sIdx] : 1.f;
        const float x = restB[size_t(v) * 3], y = restB[size_t(v) * 3 + 1], z = restB[size_t(v) * 3 + 2];
        const int32_t* jv = sk.joint + size_t(v) * size_t(K);
        const float* wv = sk.weight + size_t(v) * size_t(K);
        // every load of the vertex is issued before the first use (k < K is uniform; a padding slot names a valid joint):
        // the phase is a chain of dependent global loads on a dozen threads, so its length in round trips is what it costs
        float wAll[MMX_MAX_SKIN_INFLUENCES];
        int jAll[MMX_MAX_SKIN_INFLUENCES];
#pragma unroll
        for (int k = 0; k < MMX_MAX_SKIN_INFLUENCES; ++k) {
          wAll[k] = k < K ? wv[k] : 0.f;
          jAll[k] = k < K ? jv[k] : 0;
        }
#pragma unroll
        for (int k = 0; k < MMX_MAX_SKIN_INFLUENCES; ++k) {
          if (k >= K) {
            break;
          }
          const float wk = wAll[k];
          if (wk != 0.f) {
            const int j = jAll[k];
            const float4* M = reinterpret_cast<const float4*>(t.M) + 3 * j;
            const float4 r0 = M[0], r1 = M[1], r2 = M[2];
            const float px = r0.x * x + r0.y * y + r0.z * z + r0.w, py = r1.x * x + r1.y * y + r1.z * z + r1.w, pz = r2.x * x + r2.y * y + r2.z * z + r2.w;
            ox += wk * px, oy += wk * py, oz += wk * pz;
            iTin[k] = t.tin[j], iCoef[k] = beta * wk;
            iY[3 * k] = px, iY[3 * k + 1] = py, iY[3 * k + 2] = pz;
          } else { // padding: under no source
            iTin[k] = -1, iCoef[k] = 0.f;
            iY[3 * k] = 0.f, iY[3 * k + 1] = 0.f, iY[3 * k + 2] = 0.f;
          }
        }
      }
      t.cOut[3 * it] = beta * ox, t.cOut[3 * it + 1] = beta * oy, t.cOut[3 * it + 2] = beta * oz;
      if (sIdx == 0) {
        t.cAct[ci] = act ? 1 : 0;
      }
    }
    __syncthreads();
    // ---- S2: one row per thread: the point, the residual, sigma
    if (tid < kSneTileRows) {
      const int row = row0 + tid;
      float res = 0.f, sig = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
      if (row < rowEnd) {
        const int c = plane ? row : row / 3, k = row - 3 * c, ci = c - c0;
        if (t.cAct[ci] != 0) {
          const float* o = t.cOut + 3 * ci * S;
          float x = o[0], y = o[1], z = o[2];
          for (int q = 1; q < S; ++q) {
            x += o[3 * q], y += o[3 * q + 1], z += o[3 * q + 2];
          }
          const float dx = x - tgtB[size_t(c) * 3], dy = y - tgtB[size_t(c) * 3 + 1], dz = z - tgtB[size_t(c) * 3 + 2];
          const double s2 = double(vc.fw) * double(wB != nullptr ? wB[c] : 1.f);
          sig = float(sqrt(s2));
          float f;
          if (plane) {
            const float ax = nrmB[size_t(c) * 3], ay = nrmB[size_t(c) * 3 + 1], az = nrmB[size_t(c) * 3 + 2];
            f = ax * dx + ay * dy + az * dz;
            nx = sig * ax, ny = sig * ay, nz = sig * az;
          } else {
            f = k == 0 ? dx : (k == 1 ? dy : dz);
          }
          res = sig * f;
          errAcc += s2 * (double(f) * double(f));
        }
      }
      t.rowRes[tid] = res, t.rowSig[tid] = sig;
      t.rowN[3 * tid] = nx, t.rowN[3 * tid + 1] = ny, t.rowN[3 * tid + 2] = nz;
    }
    __syncthreads();
    // ---- T: one (constraint, column) per thread
    for (int it = tid; it < nCons * nPad; it += kT) {
      const int ci = it / nPad, col = it - ci * nPad;
      const bool act = col < n && t.cAct[ci] != 0;
      F3 D{0.f, 0.f, 0.f};
      if (act) {
        const int* iTin = t.infTin + ci * nInf;
        const float* iCoef = t.infCoef + ci * nInf;
        const float* iY = t.infY + 3 * ci * nInf;
        const int e1 = t.colRange[2 * col + 1];
        for (int e = t.colRange[2 * col]; e < e1; ++e) {
          const float* sr = t.src + kSrcRec * e;
          const int lo = __float_as_int(sr[0]), hi = __float_as_int(sr[1]), dof = __float_as_int(sr[2]);
          float m0 = 0.f, mx = 0.f, my = 0.f, mz = 0.f;
          for (int i = 0; i < nInf; ++i) {
            const int p = iTin[i];
            const bool under = p >= lo && p < hi;
            const float cf = under ? iCoef[i] : 0.f;
            m0 += cf;
            mx += under ? cf * iY[3 * i] : 0.f, my += under ? cf * iY[3 * i + 1] : 0.f, mz += under ? cf * iY[3 * i + 2] : 0.f;
          }
          const F3 ax{sr[7], sr[8], sr[9]};
          const F3 d{mx - m0 * sr[4], my - m0 * sr[5], mz - m0 * sr[6]};
          const F3 dv = dof < 3 ? m0 * ax : (dof < 6 ? cross(ax, d) : kLn2 * d);
          D = D + sr[3] * dv;
        }
      }
      if (plane) {
        const float* nr = t.rowN + 3 * ci;
        t.tile[ci * nPad + col] = act ? nr[0] * D.x + nr[1] * D.y + nr[2] * D.z : 0.f;
      } else {
        const int r = 3 * (c0 + ci) - row0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (r + k >= 0 && r + k < kSneTileRows) {
            const float dk = k == 0 ? D.x : (k == 1 ? D.y : D.z);
            t.tile[(r + k) * nPad + col] = act ? t.rowSig[r + k] * dk : 0.f;
          }
        }
      }
    }
    if (rowEnd - row0 < kSneTileRows) { // the last tile's rows past the end: exact zeros
      for (int i = (rowEnd - row0) * nPad + tid; i < kSneTileRows * nPad; i += kT) {
        t.tile[i] = 0.f;
      }
    }
    __syncthreads();
    // ---- H: tile^T tile on the matrix cores; lane l feeds row (l & 31) of A and column (l & 31) of B at k = l >> 5
    if (H != nullptr) {
#pragma unroll
      for (int q = 0; q < kSneMaxBlocksPerWave; ++q) {
        if (wave + 4 * q < numBlocks) {
          const float* ta = t.tile + (lane >> 5) * nPad + 32 * bI[q] + (lane & 31);
          const float* tb = t.tile + (lane >> 5) * nPad + 32 * bJ[q] + (lane & 31);
#pragma unroll
          for (int k = 0; k < kSneTileRows / 2; ++k) {
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[2 * k * nPad], tb[2 * k * nPad], acc[q], 0, 0, 0);
          }
        }
      }
    }
    // ---- g: (column, half of the rows) per thread, in double, rows ascending
    if (g != nullptr && gCol < n) {
      const float* tc = t.tile + gCol;
#pragma unroll 4
      for (int r = 16 * gHalf; r < 16 * gHalf + 16; ++r) {
        gAcc += double(tc[r * nPad]) * double(t.rowRes[r]);
      }
    }
    __syncthreads();
  }

  // ---- store.  D[row][col] of a block: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (kSplit) {
    if (H != nullptr) {
      float* accWs = reinterpret_cast<float*>(sp.base + sp.ws.accOffset);
#pragma unroll
      for (int q = 0; q < kSneMaxBlocksPerWave; ++q) {
        if (wave + 4 * q < numBlocks) {
          float* o = accWs + sp.ws.accIndex(b, part, wave + 4 * q) + lane;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            o[64 * r] = acc[q][r];
          }
        }
      }
    }
  } else if (H != nullptr) {
    float* Hb = H + size_t(b) * size_t(n) * size_t(n);
#pragma unroll
    for (int q = 0; q < kSneMaxBlocksPerWave; ++q) {
      if (wave + 4 * q < numBlocks) {
        const int cj = 32 * bJ[q] + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ri = 32 * bI[q] + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (ri < n && cj < n) {
            Hb[size_t(ri) * n + cj] = acc[q][r];
            if (bI[q] != bJ[q]) {
              Hb[size_t(cj) * n + ri] = acc[q][r];
            }
          }
        }
      }
    }
  }
  double* gPart = t.red;
  double* ePart = t.red + 2 * kSkinNeMaxSolved;
  gPart[gHalf * kSkinNeMaxSolved + gCol] = gAcc;
  if (tid < kSneTileRows) {
    ePart[tid] = errAcc;
  }
  __syncthreads();
  if (kSplit) {
    if (g != nullptr && tid < n) {
      reinterpret_cast<double*>(sp.base + sp.ws.gOffset)[sp.ws.gIndex(b, part) + tid] = gPart[tid] + gPart[kSkinNeMaxSolved + tid];
    }
    if (err != nullptr && tid == 0) {
      double e = 0.0;
      for (int r = 0; r < kSneTileRows; ++r) {
        e += ePart[r];
      }
      reinterpret_cast<double*>(sp.base + sp.ws.errOffset)[sp.ws.errIndex(b, part)] = e;
    }
    return;
  }
  if (g != nullptr && tid < n) {
    g[size_t(b) * n + tid] = float(gPart[tid] + gPart[kSkinNeMaxSolved + tid]);
  }
  if (err != nullptr && tid == 0) {
    double e = 0.0;
    for (int r = 0; r < kSneTileRows; ++r) {
      e += ePart[r];
    }
    err[b] = e;
  }
}

// The second pass of the split: one thread per entry of the lower block triangle (as the waves held it: [block][reg][lane]),
// per g column and per instance error.  Each sums its entry over the parts ascending, in double, rounds once and stores the
// entry (and, off the diagonal blocks, its mirror: H is bitwise symmetric as in the unsplit kernel, whose diagonal blocks are
// symmetric by the order of their products).  Consecutive threads read consecutive addresses of every part.
__global__ void __launch_bounds__(kSneThreads) skinNormalEquationsReduceKernel(
    SkinNeWorkspace ws, const char* __restrict__ base, int n, float* __restrict__ H, float* __restrict__ g, double* __restrict__ err) {
  const int accEntries = ws.numBlocks * kSkinNeBlockFloats;
  const int groups = (accEntries + ws.nPad + 1 + kSneThreads - 1) / kSneThreads; // workgroups of an instance
  const int b = int(blockIdx.x) / groups;
  const int e = (int(blockIdx.x) - b * groups) * kSneThreads + threadIdx.x;
  if (e < accEntries) {
    if (H == nullptr) {
      return;
    }
    const int block = e >> 10, r = (e >> 6) & 15, lane = e & 63;
    const float* src = reinterpret_cast<const float*>(base + ws.accOffset) + ws.accIndex(b, 0, block) + (e & (kSkinNeBlockFloats - 1));
    const int64_t stride = int64_t(ws.numBlocks) * kSkinNeBlockFloats;
    double sum = 0.0;
    for (int p = 0; p < ws.parts; ++p) {
      sum += double(src[p * stride]);
    }
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= block) {
      ++I;
    }
    const int Jb = block - I * (I + 1) / 2;
    const int cj = 32 * Jb + (lane & 31), ri = 32 * I + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (ri < n && cj < n) {
      float* Hb = H + size_t(b) * size_t(n) * size_t(n);
      const float v = float(sum);
      Hb[size_t(ri) * n + cj] = v;
      if (I != Jb) {
        Hb[size_t(cj) * n + ri] = v;
      }
    }
  } else if (e < accEntries + ws.nPad) {
    const int col = e - accEntries;
    if (g != nullptr && col < n) {
      const double* src = reinterpret_cast<const double*>(base + ws.gOffset) + ws.gIndex(b, 0) + col;
      double sum = 0.0;
      for (int p = 0; p < ws.parts; ++p) {
        sum += src[size_t(p) * ws.nPad];
      }
      g[size_t(b) * n + col] = float(sum);
    }
  } else if (e == accEntries + ws.nPad && err != nullptr) {
    const double* src = reinterpret_cast<const double*>(base + ws.errOffset) + ws.errIndex(b, 0);
    double sum = 0.0;
    for (int p = 0; p < ws.parts; ++p) {
      sum += src[p];
    }
    err[b] = sum;
  }
}

size_t skinNormalEquationsLdsBytes(int J, int P, int n, int nsrc, int S, int K) {
  return skinNeLdsFloats(J, P, n, nsrc, S, K, nullptr, nullptr) * sizeof(float);
}

hipError_t launchSkinNormalEquations(
    const RigDev& rig, const SkinNeColumnsDev& cols, const SkinDev& sk, const VertexConstraintsDev& vc, int B, const float* theta, float* H,
    float* g, double* err, hipStream_t stream) {
  const size_t lds = skinNormalEquationsLdsBytes(rig.J, rig.P, cols.n, cols.nsrc, vc.S, sk.K);
  if (lds > 160 * 1024 - 64 || B <= 0 || cols.n < 1 || cols.n > kSkinNeMaxSolved) {
    return hipErrorInvalidValue;
  }
  static LdsLimitCache ldsLimit;
  hipError_t rc = ldsLimit.ensure(reinterpret_cast<const void*>(skinNormalEquationsKernel<false>), lds);
  if (rc != hipSuccess) {
    return rc;
  }
  hipLaunchKernelGGL(skinNormalEquationsKernel<false>, dim3(B), dim3(kSneThreads), lds, stream, rig, cols, sk, vc, theta, H, g, err, SkinNeSplitDev{});
  return hipGetLastError();
}

hipError_t launchSkinNormalEquationsSplit(
    const RigDev& rig, const SkinNeColumnsDev& cols, const SkinDev& sk, const VertexConstraintsDev& vc, int B, const float* theta, float* H,
    float* g, double* err, int parts, void* workspace, hipStream_t stream) {
  const int tiles = skinNeTiles(vc.type, vc.C);
  if (tiles < 1 || parts < 1) {
    return hipErrorInvalidValue;
  }
  const int pe = skinNeEffectiveParts(parts, tiles);
  if (pe <= 1) { // one part is the unsplit launch: its bits, one kernel node, no workspace
    return launchSkinNormalEquations(rig, cols, sk, vc, B, theta, H, g, err, stream);
  }
  const size_t lds = skinNormalEquationsLdsBytes(rig.J, rig.P, cols.n, cols.nsrc, vc.S, sk.K);
  SkinNeSplitDev sp{};
  if (lds > 160 * 1024 - 64 || workspace == nullptr || !skinNeWorkspaceLayout(B, cols.n, pe, &sp.ws) || int64_t(B) * pe > 0x7fffffffll) {
    return hipErrorInvalidValue;
  }
  sp.base = static_cast<char*>(workspace);
  static LdsLimitCache ldsLimit;
  hipError_t rc = ldsLimit.ensure(reinterpret_cast<const void*>(skinNormalEquationsKernel<true>), lds);
  if (rc != hipSuccess) {
    return rc;
  }
  hipLaunchKernelGGL(skinNormalEquationsKernel<true>, dim3(B * pe), dim3(kSneThreads), lds, stream, rig, cols, sk, vc, theta, H, g, err, sp);
  rc = hipGetLastError();
  if (rc != hipSuccess) {
    return rc;
  }
  const int entries = sp.ws.numBlocks * kSkinNeBlockFloats + sp.ws.nPad + 1;
  const int64_t groups = int64_t(B) * ((entries + kSneThreads - 1) / kSneThreads);
  if (groups > 0x7fffffffll) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(
      skinNormalEquationsReduceKernel, dim3(unsigned(groups)), dim3(kSneThreads), 0, stream, sp.ws, static_cast<const char*>(workspace),
      cols.n, H, g, err);
  return hipGetLastError();
}

} // namespace mmx
