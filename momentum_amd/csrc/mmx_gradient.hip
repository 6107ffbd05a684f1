// mmx_gradient.hip -- mmx_eval_gradient: the error and the gradient 2 J^T r of every instance without a Jacobian
// (gfx950 / CDNA4, wave64).  SkeletonSolverFunctionT::getGradient (error_function_helpers.cpp:220) in O(joints + constraints).
//
// One 256-thread workgroup per instance, state in LDS; the adjoint half of treeRefineKernel (mmx_fused.hip) with d = 0 and
// lambda = 0, behind the forward kinematics and the units of treeNormalEquationsKernel:
//
//   A, B  forward kinematics, pointer-jumping rounds in double (blockFk: the solve kernels' own, so the error is the one
//         a solve reports at these parameters)
//   C     units: residual, sigma, error (in double); per unit the first-order moments of sigma^2 f (kC1 = 7 channels F | N | D)
//   D     own sums per joint by DFS position, subtree sums on the matrix cores (treeSumT<kC1, true>)
//   F     per solved column the sum of weight x sourceGradientT over its sources in table order, plus the parameter-space
//         rows (limits, model-parameter prior) evaluated on the fly from theta; x 2, scattered through the solve list
//
// No second-order channels, no H, no factor.  Every output entry is summed by one thread in a fixed order and no instance
// reads another's data: a row of the result depends on that instance's inputs only.  The gradient half is skipped as a
// whole (a workgroup-uniform branch, the same machine code in front of it) when only the error is asked for.
// The formulas are derived and validated against the explicit Jacobian in tests/tree_algebra_np.py (jt_times).
#include "mmx_device.hpp"
#include "mmx_fused_helpers.hpp"
#include "mmx_kernels.hpp"
#include "mmx_tree.hpp"

namespace mmx {

struct GradLds {
  float *th, *js, *jd, *own1, *sub1, *out;
  double *fkA, *fkB, *red;
  int *subSize, *loadedPos, *posUnitStart, *posUnits, *kRange;
};

// J: RigDev::layoutJ (the full rig's joint count: the host sizes the launch with it)
__host__ __device__ inline size_t gradientLdsFloats(int J, int P, int U, GradLds* out, float* base) {
  size_t off = 0;
  auto take = [&](size_t count) {
    const size_t o = off;
    off += alignUp4(count);
    return o;
  };
  const size_t oTh = take(P), oJs = take(size_t(kJs) * J), oFk = take(fkBufFloats(J));
  // one region, two lives: the second buffer of the pointer-jumping FK with the joint parameters in its head (read before the
  // first jump round writes there), then the own sums | the per-unit moments and, over them, the subtree sums
  const size_t own = alignUp4(size_t(kC1) * J), mom = alignUp4(size_t(kC1) * (U > J ? U : J));
  const size_t oR = take(fkBufFloats(J) > own + mom ? fkBufFloats(J) : own + mom);
  const size_t oOut = take(P);
  const size_t oSub = take(J), oLoaded = take(J), oPus = take(size_t(J) + 1), oPu = take(U), oKr = take(2 * ((size_t(J) + 15) / 16));
  const size_t oRed = take(8); // one double per wave
  if (out != nullptr) {
    out->th = base + oTh, out->js = base + oJs;
    out->fkA = reinterpret_cast<double*>(base + oFk), out->fkB = reinterpret_cast<double*>(base + oR);
    out->jd = base + oR, out->own1 = base + oR, out->sub1 = base + oR + own;
    out->out = base + oOut;
    out->subSize = reinterpret_cast<int*>(base + oSub), out->loadedPos = reinterpret_cast<int*>(base + oLoaded);
    out->posUnitStart = reinterpret_cast<int*>(base + oPus), out->posUnits = reinterpret_cast<int*>(base + oPu);
    out->kRange = reinterpret_cast<int*>(base + oKr);
    out->red = reinterpret_cast<double*>(base + oRed);
  }
  return off;
}

__global__ void __launch_bounds__(256) evalGradientKernel(
    RigDev rig,
    ProblemDev pb,
    FusedDev fd,
    const float* __restrict__ theta, // [B][P]
    float* __restrict__ grad, // [B][P] every entry written, or null: the error only
    double* __restrict__ errOut) { // [B] or null
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int kT = 256, kWaves = 4;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  selectInstanceRig(rig, b);
  selectInstanceWeights(pb, b);
  const int J = rig.J, P = rig.P, U = fd.U, n = fd.n;
  const bool wantGrad = grad != nullptr; // (uniform)
  GradLds t;
  gradientLdsFloats(rig.layoutJ, P, U, &t, smem);
  FusedLds s{};
  s.th = t.th, s.js = t.js, s.fkA = t.fkA, s.fkB = t.fkB, s.jd = t.jd, s.own1 = t.own1, s.sub1 = t.sub1, s.red = t.red;
  RigView rv;
  rv.J = J, rv.P = P, rv.R = rig.R, rv.numLevels = rig.numLevels, rv.jumpRounds = rig.jumpRounds;
  rv.parent = rig.parent, rv.preRot = rig.preRot, rv.offset = rig.offset;
  rv.ptOuter = rig.ptOuter, rv.ptInner = rig.ptInner, rv.ptValue = rig.ptValue, rv.ptOffsets = rig.ptOffsets;
  rv.hasOffsets = rig.ptOffsetsNonZero != 0;
  rv.levelOrder = rig.levelOrder, rv.levelStart = rig.levelStart;
  rv.rowRec = rig.ptRowRec, rv.numRowRec = rig.numRowRec;
  FusedView fv;
  fv.U = U, fv.Kp = fd.Kp, fv.subSize = t.subSize, fv.dfsJoint = fd.dfsJoint, fv.loadedPos = t.loadedPos, fv.numLoaded = fd.numLoaded;
  fv.colToSolve = nullptr, fv.unitPos = pb.unitTin, fv.posUnitStart = t.posUnitStart, fv.posUnits = t.posUnits, fv.solveList = fd.solveList;
  for (int i = tid; i < P; i += kT) {
    s.th[i] = theta[size_t(b) * P + i];
  }
  if (wantGrad) {
    for (int i = tid; i < P; i += kT) {
      t.out[i] = 0.f; // disabled parameters and structurally zero columns: exact zeros
    }
    for (int i = tid; i < J; i += kT) {
      t.subSize[i] = fd.subSize[i];
      t.loadedPos[i] = i < fd.numLoaded ? fd.loadedPos[i] : 0;
    }
    for (int i = tid; i <= J; i += kT) {
      t.posUnitStart[i] = fd.posUnitStart[i];
    }
    for (int i = tid; i < U; i += kT) {
      t.posUnits[i] = fd.posUnits[i];
    }
  }
  __syncthreads();
  if (wantGrad) {
    treeSumRanges(t.subSize, t.loadedPos, fv.numLoaded, J, tid, t.kRange); // (barriers follow before the tree sum)
  }
  // the thread's first unit: requested before the forward kinematics (treeNormalEquationsKernel)
  const UnitInput uin0 = loadUnitInput(pb, b, tid < U ? tid : U);
  // ---- A, B: forward kinematics; the rotation axes only where the gradient reads them
  blockFk<true, kT>(rv, s, s.th, tid, wantGrad);
  // ---- C: units; the moments of y = sigma^2 f land in the scratch the subtree sums overwrite later
  double e = 0.0;
  for (int u = tid; u < U; u += kT) {
    const Unit un = evalUnitFrom(pb, u == tid ? uin0 : loadUnitInput(pb, b, u), s.js, u);
    e += double(un.werr);
    if (wantGrad) {
      const float sg2 = un.sigma * un.sigma;
      firstOrderMoments(s.sub1 + kC1 * u, un.v, sg2 * un.f.x, sg2 * un.f.y, sg2 * un.f.z, u < fd.Kp);
    }
  }
  const bool hasParamRows = pb.M > pb.rowsJoint; // limit / model-parameter rows present (uniform)
  if (hasParamRows) {
    e += paramRowsErrorT<true, float>(rig, pb, P, s.th, b, tid);
  }
  e = waveReduceSum(e);
  if (lane == 0) {
    s.red[wave] = e;
  }
  __syncthreads();
  if (errOut != nullptr && tid == 0) {
    errOut[b] = (s.red[0] + s.red[1]) + (s.red[2] + s.red[3]);
  }
  if (!wantGrad) {
    return;
  }
  // ---- D: own sums per joint (ascending unit order), then subtree sums
  gatherOwnSums<kC1, kC1, kT>(fv, s, s.sub1, tid);
  __syncthreads();
  treeSumT<kC1, true, kC1, 8>(fv.subSize, fv.loadedPos, fv.numLoaded, s.own1, s.sub1, J, wave, kWaves, lane, t.kRange);
  __syncthreads();
  // ---- F: J^T r per solved column: the primary source slot, then the extras (slot numbering of treeRefineKernel)
  for (int c = tid; c < n; c += kT) {
    auto slotShare = [&](int e2) {
      const ColumnSourceDev cs = fd.srcs[e2];
      return cs.weight * sourceGradientT(cs.joint, cs.dof, cs.parent, s.js, s.sub1 + kC1 * cs.tin);
    };
    float a = slotShare(c);
    const int e1 = fd.slotBase + fd.srcStart[c + 1];
    for (int e2 = fd.slotBase + fd.srcStart[c]; e2 < e1; ++e2) {
      a += slotShare(e2);
    }
    const int p = fd.solveList[c];
    if (hasParamRows) {
      a += paramRowsColumn<int32_t>(rig, pb, fd, s.th, nullptr, nullptr, P, b, c, p).g;
    }
    t.out[p] = 2.f * a;
  }
  __syncthreads();
  for (int i = tid; i < P; i += kT) {
    grad[size_t(b) * P + i] = t.out[i];
  }
}

size_t gradientLdsBytes(int J, int P, int U) {
  return gradientLdsFloats(J, P, U, nullptr, nullptr) * sizeof(float);
}

hipError_t launchEvalGradient(const RigDev& rig, const ProblemDev& pb, const FusedDev& fd, const float* theta, float* grad, double* err, hipStream_t stream) {
  const size_t lds = gradientLdsBytes(rig.layoutJ, rig.P, fd.U);
  if (lds > 160 * 1024 - 64 || pb.B <= 0) {
    return hipErrorInvalidValue;
  }
  static LdsLimitCache ldsLimit;
  hipError_t rc = ldsLimit.ensure(reinterpret_cast<const void*>(evalGradientKernel), lds);
  if (rc != hipSuccess) {
    return rc;
  }
  hipLaunchKernelGGL(evalGradientKernel, dim3(pb.B), dim3(256), lds, stream, rig, pb, fd, theta, grad, err);
  return hipGetLastError();
}

} // namespace mmx
