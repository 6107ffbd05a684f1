// mmx_fused_helpers.hpp -- device helpers shared by the kernels of mmx_fused.hip and mmx_gradient.hip: the LDS views, the
// per-unit moments and own sums of the adjoint pass, the parameter-space rows, the transform walks and the block forward
// kinematics.  Inline templates only: a translation unit pays for what it instantiates.
#pragma once

#include "mmx_device.hpp"
#include "mmx_kernels.hpp"
#include "mmx_tree.hpp"

namespace mmx {

struct FusedLds {
  // ---- loaded once per launch (batch-shared integer tables and the parameter-transform CSR)
  // source SLOTS: slot c < NP is the primary source of column c (pad columns: weight 0), slots >= NP are
  // the further sources of multi-source columns: extras of column c = NP + mStart[c] .. NP + mStart[c+1] - 1
  int16_t* mStart; // [NP+1] column -> number of extra slots before it
  int* mTin; // [nsrc] DFS interval of the slot's joint: tin | tout << 16
  int* mInfo; // [nsrc] joint | dof << 12 | (parent + 1) << 16
  float* mW; // [nsrc]
  // ---- per iteration
  float* th; // [P] theta (full parameter space)
  float* js; // [kJs J] world t(3) q(4) s(1) | rotation axes (9)
  float* up; // [3 U] unit world vector
  float* ur; // [3 U] scaled residual rows r
  float* uy; // [3 U] sigma * (r or w): input of the adjoint pass
  float* us; // [U]   sigma
  float* own1; // [kC1 J] first-order sums over the joint's own units (by DFS position)
  float* sub1; // [kC1 J] ... over the joint's subtree
  float* g; // [NP]
  float* d0; // [NP]
  float* rho; // [NP]
  float* invDiag; // [NP] 1 / L(i,i)
  float* dfull; // [P]
  float* jd; // [7 J]
  float* tanOwn; // [kTan J]
  float* tanPre; // [kTan J]
  double* red; // [8]
  int* flags; // [4]: stop | not positive definite (this iteration) | status | unused
  // ---- rows of the further joint error functions and ellipsoid limits (kGen instantiations): dense in LDS
  float* gEv; // [GT][kGenEv] per constraint: vp(3) vn(3) sigma*dp(9) sigma*dn(9) tin row flags tinStop (pair constraints: the second point's tin)
  float* gRes; // [rowsGp] residual rows
  float* gW; // [rowsGp] r - J d of the refinement
  float* gJ; // [rowsGp][gst] their Jacobian rows over the solve columns (pad rows / columns zero)
  // ---- one region, two lives: assembly scratch (phases A-G), then the Cholesky factor (H-J)
  double* fkA; // [kFkCh][fkPad(J)] the two buffers of the pointer-jumping FK (mmx_device.hpp fkJumpRoundsD); fkB lies over
  double* fkB; // own2 / sub2, which phase D writes after FK is done
  float* own2; // [kC2 J]
  float* umom; // [kUmom U] per-unit moment contributions (phase D only)
  float* sub2; // [kC2 J]
  float* L; // [T][256] tiles; a diagonal tile holds L_kk (lower triangle) and L_kk^-T (strict upper triangle)
  // ---- aliases the refinement scratch (dfull, jd, tanOwn, tanPre): dead before phase J starts
  float* srcT; // one-launch solve: [nsrc][kSlotStride] slot-major, per slot weighted D (7 channels) | weighted A (7); the tree
  // kernels: [15][srcStride] channel-major, weighted D (7) | weighted A (7) | weighted J^T r share (1)
};

// Views of the batch-shared tables after they were copied into LDS.  Plain local structs whose
// pointers come straight from the LDS carve, so the compiler keeps the LDS address space (ds_read)
// instead of falling back to flat loads.
struct RigView {
  int32_t J, P, R, numLevels, jumpRounds;
  const int32_t* parent;
  const float* preRot; // stays in global memory (read once per joint per iteration)
  const float* offset; // "
  const int32_t* ptOuter;
  const int32_t* ptInner;
  const float* ptValue;
  const float* ptOffsets; // "
  bool hasOffsets; // some entry of ptOffsets is non-zero (RigDev::ptOffsetsNonZero)
  const int32_t* levelOrder;
  const int32_t* levelStart;
  const int4* rowRec; // RigDev::ptRowRec (null: walk the CSR)
  int32_t numRowRec;
};
// I: int32_t where the tables stay in global memory or are LDS copies of the tree kernels; int16_t in the one-launch solve,
// whose LDS budget is what decides between three and four workgroups per CU (every index of a fused problem is below 4096)
template <class I>
struct FusedViewT {
  int32_t U, Kp;
  const I* subSize;
  const I* dfsJoint;
  const I* loadedPos;
  int32_t numLoaded;
  const I* colToSolve; // [P] compacted index of a parameter or -1
  const I* unitPos; // [U] DFS position of the joint a unit hangs on
  const I* posUnitStart;
  const I* posUnits;
  const I* solveList;
};
using FusedView = FusedViewT<int32_t>;
using FusedViewS = FusedViewT<int16_t>;

__host__ __device__ __forceinline__ size_t alignUp4(size_t x) {
  return (x + 3) & ~size_t(3);
}
// channel stride of the per-slot tables: >= nsrc and = 16 mod 32, so that the 16 slots x 2 channels a
// 32-lane group reads as MFMA operands (phase G) fall into 32 different banks
__host__ __device__ __forceinline__ int srcStrideFor(int nsrc) {
  int x = (nsrc + 15) & ~15;
  return (x & 31) == 16 ? x : x + 16;
}
constexpr int kSrcCh = 15; // D(7) | A(7) | g share (the tree kernels; the one-launch solve keeps the g share in uy's place: 14)
// The one-launch solve's slot tables are SLOT-major with a compile-time stride: D channels at 0..6, A channels at 7..13 of a
// slot, so that every access is one per-slot address plus an immediate (a run-time channel stride cost fourteen SGPR bases
// per term record, which spilled).  14 keeps the MFMA operand loads of phase G -- 16 slots x 2 adjacent channels per 32
// lanes -- in 32 different banks (14 i mod 32 takes the sixteen even values); phase E's per-slot stores are two-way.
constexpr int kSlotStride = 14;
__host__ __device__ __forceinline__ size_t slotTableFloats(int nsrc) { // never more than (kSrcCh - 1) * srcStrideFor(nsrc)
  return size_t(kSlotStride) * size_t((nsrc + 15) & ~15);
}

// ---------------------------------------------------------------------------------------------
// adjoint machinery: sums over a joint's own units, then over its subtree (= a DFS index range)
// ---------------------------------------------------------------------------------------------
// Two steps, both fully parallel: (1) one thread per unit writes the unit's moment contributions
// (NCH floats: kC1 first-order, then kC2 second-order channels) to a scratch array; (2) one thread per
// (loaded joint, channel) adds up the few units of that joint, in ascending unit order.  Joints
// without units are never read by the subtree sums (treeSumT walks loadedPos), so they are skipped.
__device__ __forceinline__ void firstOrderMoments(float* o, F3 p, float yx, float yy, float yz, bool point) {
  // N += p x y (points and directions share the channel: only the sum enters, see jt_times)
  o[3] = p.y * yz - p.z * yy;
  o[4] = p.z * yx - p.x * yz;
  o[5] = p.x * yy - p.y * yx;
  o[0] = point ? yx : 0.f;
  o[1] = point ? yy : 0.f;
  o[2] = point ? yz : 0.f;
  o[6] = point ? p.x * yx + p.y * yy + p.z * yz : 0.f;
}

// NCH channels per unit (kC1 first-order, then kC2Used second-order ones), stored with stride STRIDE (odd)
template <int NCH, int STRIDE, int kT = 256, class FV = FusedView, bool kSecondOnly = false>
__device__ __forceinline__ void gatherOwnSums(const FV& fd, const FusedLds& s, const float* umom, int tid) {
  for (int item = tid; item < fd.numLoaded * NCH; item += kT) {
    const int li = item / NCH, c = item - li * NCH;
    const int k = fd.loadedPos[li];
    float acc = 0.f;
    const int e1 = fd.posUnitStart[k + 1];
    for (int e = fd.posUnitStart[k]; e < e1; ++e) {
      acc += umom[STRIDE * fd.posUnits[e] + c];
    }
    if (kSecondOnly) { // (the channels are the second-order ones only)
      s.own2[kC2 * k + c] = acc;
    } else if (c < kC1) {
      s.own1[kC1 * k + c] = acc;
    } else {
      s.own2[kC2 * k + (c - kC1)] = acc;
    }
  }
}
constexpr int kUmom = 25; // stride of the per-unit moment scratch: 7 + 16 channels, odd

// phase D: first- and second-order own sums from up / uy / us
// kSecondOnly: the second-order channels only (the mixed-precision solve: g = J^T r is formed in double, mmx_mixed.hpp; uy is
// not read)
// (upD / usD: the units' vectors and weights in double, rounded here -- the mixed route keeps no single-precision copies)
template <int kT = 256, class FV = FusedView, bool kSecondOnly = false>
__device__ __forceinline__ void ownSums(const FV& fd, const FusedLds& s, float* umom, int U, int tid, const double* upD = nullptr, const double* usD = nullptr) {
  constexpr int NCH = kSecondOnly ? kC2Used : kC1 + kC2Used;
  for (int u = tid; u < U; u += kT) {
    const F3 p = kSecondOnly ? F3{float(upD[3 * u]), float(upD[3 * u + 1]), float(upD[3 * u + 2])} : F3{s.up[3 * u], s.up[3 * u + 1], s.up[3 * u + 2]};
    const bool point = u < fd.Kp;
    float* o = umom + kUmom * u;
    if (!kSecondOnly) {
      firstOrderMoments(o, p, s.uy[3 * u], s.uy[3 * u + 1], s.uy[3 * u + 2], point);
    }
    const float sg = kSecondOnly ? float(usD[u]) : s.us[u];
    const float s2 = sg * sg;
    float* o2 = kSecondOnly ? o : o + kC1;
#pragma unroll
    for (int c = 0; c < kC2Used; ++c) {
      o2[c] = 0.f;
    }
    const int q = point ? 4 : 10;
    o2[q + 0] = s2 * p.x * p.x;
    o2[q + 1] = s2 * p.x * p.y;
    o2[q + 2] = s2 * p.x * p.z;
    o2[q + 3] = s2 * p.y * p.y;
    o2[q + 4] = s2 * p.y * p.z;
    o2[q + 5] = s2 * p.z * p.z;
    if (point) {
      o2[0] = s2;
      o2[1] = s2 * p.x;
      o2[2] = s2 * p.y;
      o2[3] = s2 * p.z;
    }
  }
  __syncthreads();
  gatherOwnSums<NCH, kUmom, kT, FV, kSecondOnly>(fd, s, umom, tid);
}

constexpr int kFusedTreeUn = 4; // k-steps per trip of the tree sums (measured on BASELINE configs[1]: 1 -> 1.575e6, 4 -> 1.60e6, 8 -> 1.54e6 solves/s)
template <int NC, bool kSubtree, int STRIDE = NC, int UN = kFusedTreeUn, class I = int32_t>
__device__ __forceinline__ void treeSum(const FusedViewT<I>& fd, const float* in, float* out, int J, int wave, int lane, const int32_t* kRange = nullptr) {
  treeSumT<NC, kSubtree, STRIDE, UN, I>(fd.subSize, fd.loadedPos, fd.numLoaded, in, out, J, wave, 4, lane, kRange);
}

// ---------------------------------------------------------------------------------------------
// parameter-space rows (LimitErrorFunctionT on model parameters, ModelParametersErrorFunctionT):
// they need no joint state, so their contributions to the error, to g / H and to the refinement
// are evaluated on the fly from theta -- no extra LDS, nothing stored per row.
// ---------------------------------------------------------------------------------------------
struct ParamCol {
  float g, h;
};

// contributions of the rows to solve column c = parameter p: g_c = sum_l J(l,c) r_l and
// H_cc = sum_l J(l,c)^2.  With a step `d0` the residual is replaced by r - J d0 (refinement).
template <class I = int32_t>
__device__ __forceinline__ ParamCol paramRowsColumn(
    const RigDev& rig,
    const ProblemDev& pb,
    const FusedDev& fd,
    const float* th,
    const float* d0,
    const I* colToSolve,
    int P,
    int b,
    int c,
    int p) {
  ParamCol o{0.f, 0.f};
  if (fd.numLimits > 0 && pb.wLimit > 0.f) {
    const float tWeight = 1e+1f * pb.wLimit;
    const int k1 = fd.limStart[c + 1];
    for (int k = fd.limStart[c]; k < k1; ++k) {
      const LimitRow row = evalLimit(rig, pb.limits[fd.limOf[k]], th, pb.enabledMask, tWeight);
      float coef = 0.f, rr = row.r;
#pragma unroll
      for (int e = 0; e < kLimitEntries; ++e) {
        coef += row.idx[e] == p ? row.coef[e] : 0.f;
        if (d0 != nullptr) {
          const int sc = row.idx[e] >= 0 ? colToSolve[row.idx[e]] : -1;
          rr -= row.coef[e] * (sc >= 0 ? d0[sc] : 0.f); // parameters outside the solve list do not move
        }
      }
      o.g += coef * rr;
      o.h += coef * coef;
    }
  }
  if (pb.hasModel && pb.wModel > 0.f) {
    const float w = pb.mpWeights[size_t(b) * P + p];
    if (w > 0.f) {
      const float sWeight = sqrtf(pb.wModel * 1e-1f);
      const float a = sWeight * w;
      float rr = (w * (th[p] - pb.mpTarget[size_t(b) * P + p])) * sWeight;
      if (d0 != nullptr) {
        rr -= a * d0[c];
      }
      o.g += a * rr;
      o.h += a * a;
    }
  }
  return o;
}

// The same in double for the mixed-precision instantiation (LimitErrorFunctionT<double>, ModelParametersErrorFunctionT<double>):
// kOp = false: g_c = sum_l J(l,c) r_l and H_cc = sum_l J(l,c)^2 of the rows at theta `th`; kOp = true: the rows' part of the
// operator, (J_p^T J_p x)_c for the vector x over the solve columns (g) -- h unused.
struct ParamColD {
  double g, h;
};
template <bool kOp, class I>
__device__ __forceinline__ ParamColD paramRowsColumnD(
    const RigDev& rig, const ProblemDev& pb, const FusedDev& fd, const double* th, const double* x, const I* colToSolve, int P, int b, int c, int p) {
  ParamColD o{0.0, 0.0};
  if (fd.numLimits > 0 && pb.wLimit > 0.f) {
    const double tWeight = double(1e+1f * pb.wLimit); // kLimitWeight * weight_ (a float product in both instantiations)
    const int k1 = fd.limStart[c + 1];
    for (int k = fd.limStart[c]; k < k1; ++k) {
      const LimitRowT<double> row = evalLimit<double>(rig, pb.limits[fd.limOf[k]], th, pb.enabledMask, tWeight);
      double coef = 0.0, jx = 0.0;
#pragma unroll
      for (int e = 0; e < kLimitEntries; ++e) {
        coef += row.idx[e] == p ? row.coef[e] : 0.0;
        if (kOp) {
          const int sc = row.idx[e] >= 0 ? colToSolve[row.idx[e]] : -1;
          jx += row.coef[e] * (sc >= 0 ? x[sc] : 0.0); // parameters outside the solve list do not move
        }
      }
      o.g += coef * (kOp ? jx : row.r);
      o.h += coef * coef;
    }
  }
  if (pb.hasModel && pb.wModel > 0.f) {
    const double w = double(pb.mpWeights[size_t(b) * P + p]);
    if (w > 0.0) {
      const double sWeight = double(sqrtf(pb.wModel * 1e-1f)); // sWeight: a float in both instantiations (model_parameters_error_function.cpp:109)
      const double a = sWeight * w;
      o.g += a * (kOp ? a * x[c] : (w * (th[p] - double(pb.mpTarget[size_t(b) * P + p]))) * sWeight);
      o.h += a * a;
    }
  }
  return o;
}
// y = A x for a CSR matrix whose tables live in GLOBAL memory (the wide kernels; the fused solve keeps them in LDS):
// four rows per trip with their row bounds, then their first entries, requested together -- a row's walk is a chain
// of dependent L2 round trips otherwise.  Same products in the same order as the plain walk.
template <int kT = 256, typename Gather, typename Store> // kT: threads of the workgroup
__device__ __forceinline__ void csrRowsPrefetched(const int32_t* outer, const int32_t* inner, const float* value, int R, int tid, Gather x, Store out) {
  for (int r0 = tid; r0 < R; r0 += 4 * kT) {
    int ka[4], kb[4], in0[4];
    float v0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = min(r0 + kT * i, R - 1);
      ka[i] = outer[r], kb[i] = outer[r + 1];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool has = kb[i] > ka[i];
      in0[i] = has ? inner[ka[i]] : 0, v0[i] = has ? value[ka[i]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + kT * i;
      if (r < R) {
        decltype(x(0)) acc = 0; // (float; double in the mixed-precision solve)
        if (kb[i] > ka[i]) {
          acc += v0[i] * x(in0[i]);
          for (int k = ka[i] + 1; k < kb[i]; ++k) {
            acc += value[k] * x(inner[k]);
          }
        }
        out(r, acc);
      }
    }
  }
}

// y = A x from the records of A's non-empty rows (RigDev::ptRowRec): one 16-byte load per thread, then a row's first product
// from the record itself; the rare further entries of a row from the CSR arrays.  out(r, value) is called for EVERY row r < R
// exactly once (the empty ones with 0) by the thread that owns the record before it -- no zero-fill pass, no barrier.
template <int kT = 256, typename Gather, typename Store>
__device__ __forceinline__ void csrRowsFromRecords(const int4* rec, int numRec, const int32_t* inner, const float* value, int R, int tid, Gather x, Store out) {
  for (int t = tid; t < numRec; t += kT) {
    const int4 q = rec[t];
    const int row = q.x & 0xffff, span = int(uint32_t(q.x) >> 16), in0 = q.y & 0xffff, cnt = int(uint32_t(q.y) >> 16); // (unsigned fields: mmx_rig_create builds no records when one would not fit 16 bits)
    auto acc = __int_as_float(q.z) * x(in0); // (float; double in the mixed-precision solve)
    for (int k = q.w + 1; k < q.w + cnt; ++k) {
      acc += value[k] * x(inner[k]);
    }
    out(row, acc);
    for (int r = row + 1; r < row + span; ++r) {
      out(r, decltype(acc)(0));
    }
    if (t == 0) {
      for (int r = 0; r < row; ++r) {
        out(r, decltype(acc)(0));
      }
    }
  }
}

// Forward kinematics of the whole skeleton from the parameters in `th` into s.js: local transforms
// of all joints at once (parameter_transform.cpp:110-124, joint_state.cpp:44-62), world transforms
// by pointer jumping (skeleton_state.cpp:100-121 re-associated), optionally the rotation axes.
// Ends with a barrier.  Clobbers alt / jlA / jlB (assembly scratch = the Cholesky region).
// kUnitLocal (the skeleton state's backward pass only; the solves and the forward keep false and their code): every local
// quaternion is renormalised in double before the composition.  A single-precision local quaternion has |q_l| = 1 +- 5e-8 and
// the rounds compose exactly, so the world quaternion's norm is the PRODUCT of the local norms (1 - 8e-7 fifteen joints down
// an all-dof chain); a quaternion of norm rho turns v into (1 - rho^2) v + rho^2 R v, which puts 1 - rho^2 on every lever arm
// and axis below -- invisible to a solve at 1e-5, ten times the rounding of a derivative of the state.
template <bool kGlobalTables = false, int kT = 256, bool kUnitLocal = false> // the rig's CSR tables are read from global memory (prefetching walk); kT threads
__device__ __forceinline__ void
blockFk(const RigView& rig, const FusedLds& s, const float* th, int tid, bool withAxes, long long* clk = nullptr, long long* clkLast = nullptr) {
  auto stamp = [&](int slot) { // profiling aid (MMX_PHASE_CLOCKS): sub-phases of FK
    if (clk != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
      const long long now = clock64();
      clk[slot] += now - *clkLast;
      *clkLast = now;
    }
  };
  // joint parameters = transform * theta + offsets, one transform ROW per thread (parameter_transform.cpp:
  // 110-124; the same products in the same order as a per-joint walk): 7 J independent short CSR walks
  // instead of seven dependent ones per joint.  They land in the refinement scratch (jd), which is dead
  // whenever FK runs.
  if (kGlobalTables && rig.rowRec != nullptr) {
    csrRowsFromRecords<kT>(
        rig.rowRec, rig.numRowRec, rig.ptInner, rig.ptValue, rig.R, tid, [&](int c) { return th[c]; }, [&](int r, float acc) { s.jd[r] = acc + (rig.hasOffsets ? rig.ptOffsets[r] : 0.f); });
  } else if (kGlobalTables) {
    csrRowsPrefetched<kT>(
        rig.ptOuter, rig.ptInner, rig.ptValue, rig.R, tid, [&](int c) { return th[c]; }, [&](int r, float acc) { s.jd[r] = acc + (rig.hasOffsets ? rig.ptOffsets[r] : 0.f); });
  } else {
    for (int r = tid; r < rig.R; r += kT) {
      const float off = rig.hasOffsets ? rig.ptOffsets[r] : 0.f; // (a global load on the phase's critical path when it is taken)
      float acc = 0.f;
      const int k1 = rig.ptOuter[r + 1];
      for (int k = rig.ptOuter[r]; k < k1; ++k) {
        acc += rig.ptValue[k] * th[rig.ptInner[k]];
      }
      s.jd[r] = acc + off;
    }
  }
  // the joint's constants are requested before the barrier, so that their L2 round trip overlaps it
  float pre[4] = {0.f, 0.f, 0.f, 1.f}, off3[3] = {0.f, 0.f, 0.f};
  if (tid < rig.J) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      pre[d] = rig.preRot[4 * tid + d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      off3[d] = rig.offset[3 * tid + d];
    }
  }
  __syncthreads();
  stamp(26);
  const int Jp = fkPad(rig.J);
  for (int j = tid; j < rig.J; j += kT) {
    float* slot = s.js + kJs * j;
    float loc[8];
    if (j == tid) {
      fkLocalFromParams(s.jd + 7 * j, pre, off3, loc, slot + 8);
    } else {
      fkLocalFromParams(s.jd + 7 * j, rig.preRot + 4 * j, rig.offset + 3 * j, loc, slot + 8);
    }
    if (kUnitLocal) {
      const double qx = loc[3], qy = loc[4], qz = loc[5], qw = loc[6];
      const double inv = 1.0 / sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
      if (rig.jumpRounds == 0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          slot[c] = c >= 3 && c < 7 ? float(double(loc[c]) * inv) : loc[c];
        }
      } else {
        FkXf x;
        x.tx = loc[0], x.ty = loc[1], x.tz = loc[2], x.qx = qx * inv, x.qy = qy * inv, x.qz = qz * inv, x.qw = qw * inv;
        x.s = loc[7], x.jl = rig.parent[j] + 1;
        fkStoreD(s.fkA, Jp, j, x);
      }
    } else if (rig.jumpRounds == 0) { // every joint is a root
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        slot[c] = loc[c];
      }
    } else {
      fkStoreLocalD(s.fkA, Jp, j, loc, rig.parent[j] + 1);
    }
  }
  __syncthreads();
  stamp(24);
  fkJumpRoundsD(s.js, s.fkA, s.fkB, rig.J, rig.jumpRounds, tid, kT);
  stamp(25);
  if (withAxes) {
    for (int j = tid; j < rig.J; j += kT) {
      fkAxesInPlaceP(rig, j, rig.parent[j], s.js);
    }
    __syncthreads();
  }
}

} // namespace mmx
