// mmx_state_backward.hip -- mmx_eval_skeleton_state_backward: the vector-Jacobian product of the skeleton state
// theta -> [J][8] = (t, q, s) with a caller-supplied cotangent, without a state Jacobian (gfx950 / CDNA4, wave64).
// The backward half of pymomentum/backend/triton_fk.py (_backward_kernel) in O(joints + entries of the parameter transform).
//
// One 256-thread workgroup per instance, state in LDS; evalGradientKernel (mmx_gradient.hip) with the JOINTS as the units
// and the cotangent in the place of sigma^2 f:
//
//   A, B  forward kinematics, pointer-jumping rounds in double (blockFk: the solve kernels' own, with every local quaternion
//         renormalised in double before the rounds -- kUnitLocal), with the rotation axes
//   C     one joint per thread: from g = stateGrad[b][j] and the joint's world state (t, q, s) the seven first-order
//         channels at the joint's DFS position
//           F = g_t
//           N = t x F + tau,  tau = 1/2 Im(g_q (x) conj(q))     (dq = 1/2 (omega, 0) (x) q for a world rotation omega above j)
//           D = t . F + s g_s                                   (ds_j / dsigma_a = ln 2 s_j for every j below a, a included)
//   D     subtree sums on the matrix cores (treeSumT<kC1, true>) over all J positions
//   F     one model parameter per thread: the sum of weight x sourceGradientT over its transform entries in row order
//         (translation: axis . F_sub; rotation: axis . (N_sub - t_a x F_sub); scale: ln 2 (D_sub - t_a . F_sub)); no factor 2
//
// Every output entry is summed by one thread in a fixed order and no instance reads another's data: a row of the result
// depends on that instance's inputs only.  The formulas are derived and validated against a dense Jacobian in
// tests/skeleton_state_reference.py (channels_np / vjp_np).
//
// LDS map (floats; every piece rounded up to a multiple of 4):
//   th [P] | js [kJs J] | fkA [fkBufFloats(J)] | R | subSize [J] | loadedPos [J] | kRange [2 ceil(J / 16)]
//   R = max(fkBufFloats(J), 2 x 7 J): one region, two lives -- the second buffer of the pointer-jumping FK with the joint
//   parameters (7 J) in its head, then the own channels [7 J] | the subtree sums [7 J]
#include "mmx_device.hpp"
#include "mmx_fused_helpers.hpp"
#include "mmx_kernels.hpp"
#include "mmx_tree.hpp"

namespace mmx {

struct StateBackwardLds {
  float *th, *js, *jd, *own1, *sub1;
  double *fkA, *fkB;
  int *subSize, *loadedPos, *kRange;
};

__host__ __device__ inline size_t stateBackwardLdsFloats(int J, int P, StateBackwardLds* out, float* base) {
  size_t off = 0;
  auto take = [&](size_t count) {
    const size_t o = off;
    off += alignUp4(count);
    return o;
  };
  const size_t oTh = take(P), oJs = take(size_t(kJs) * J), oFk = take(fkBufFloats(J));
  const size_t own = alignUp4(size_t(kC1) * J);
  const size_t oR = take(fkBufFloats(J) > 2 * own ? fkBufFloats(J) : 2 * own);
  const size_t oSub = take(J), oLoaded = take(J), oKr = take(2 * ((size_t(J) + 15) / 16));
  if (out != nullptr) {
    out->th = base + oTh, out->js = base + oJs;
    out->fkA = reinterpret_cast<double*>(base + oFk), out->fkB = reinterpret_cast<double*>(base + oR);
    out->jd = base + oR, out->own1 = base + oR, out->sub1 = base + oR + own;
    out->subSize = reinterpret_cast<int*>(base + oSub), out->loadedPos = reinterpret_cast<int*>(base + oLoaded);
    out->kRange = reinterpret_cast<int*>(base + oKr);
  }
  return off;
}

__global__ void __launch_bounds__(256) skeletonStateBackwardKernel(
    RigDev rig,
    StateBackwardDev sb,
    const float* __restrict__ theta, // [B][P]
    const float* __restrict__ stateGrad, // [B][J][8]
    float* __restrict__ thetaGrad) { // [B][P] every entry written
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int kT = 256, kWaves = 4;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  selectInstanceRig(rig, b);
  const int J = rig.J, P = rig.P;
  StateBackwardLds t;
  stateBackwardLdsFloats(J, P, &t, smem);
  FusedLds s{};
  s.th = t.th, s.js = t.js, s.fkA = t.fkA, s.fkB = t.fkB, s.jd = t.jd, s.own1 = t.own1, s.sub1 = t.sub1;
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
    t.subSize[i] = sb.subSize[i];
    t.loadedPos[i] = sb.loadedPos[i];
  }
  // the thread's first joint: its cotangent and position are requested before the forward kinematics
  const float* gIn = stateGrad + size_t(b) * 8 * size_t(J);
  float g0[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    g0[c] = tid < J ? gIn[8 * tid + c] : 0.f;
  }
  const int pos0 = tid < J ? sb.jointPos[tid] : 0;
  __syncthreads();
  treeSumRanges(t.subSize, t.loadedPos, J, J, tid, t.kRange); // (barriers follow before the tree sum)
  // ---- A, B: forward kinematics with the rotation axes; the local quaternions renormalised in double (blockFk, kUnitLocal:
  // a derivative sees the norm drift of the exact composition of single-precision rotations, 1e-6 down a long chain)
  blockFk<true, kT, true>(rv, s, s.th, tid, true);
  // ---- C: the joints' channels by DFS position, over the FK's second buffer (dead since blockFk's last barrier)
  for (int j = tid; j < J; j += kT) {
    float g[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      g[c] = j == tid ? g0[c] : gIn[8 * j + c];
    }
    const int pos = j == tid ? pos0 : sb.jointPos[j];
    const float* w = s.js + kJs * j;
    const F3 tj{w[0], w[1], w[2]}, F{g[0], g[1], g[2]};
    const float qx = w[3], qy = w[4], qz = w[5], qw = w[6];
    // tau = 1/2 Im(g_q (x) conj(q)), Hamilton product in (x, y, z, w) storage
    const F3 tau{
        0.5f * (-g[6] * qx + g[3] * qw - g[4] * qz + g[5] * qy),
        0.5f * (-g[6] * qy + g[4] * qw - g[5] * qx + g[3] * qz),
        0.5f * (-g[6] * qz + g[5] * qw - g[3] * qy + g[4] * qx)};
    const F3 N = cross(tj, F) + tau;
    float* o = s.own1 + kC1 * pos;
    o[0] = F.x, o[1] = F.y, o[2] = F.z;
    o[3] = N.x, o[4] = N.y, o[5] = N.z;
    o[6] = dot(tj, F) + w[7] * g[7];
  }
  __syncthreads();
  // ---- D: subtree sums
  treeSumT<kC1, true, kC1, 8>(t.subSize, t.loadedPos, J, s.own1, s.sub1, J, wave, kWaves, lane, t.kRange);
  __syncthreads();
  // ---- F: per model parameter, its transform entries in row order
  for (int p = tid; p < P; p += kT) {
    float a = 0.f;
    const int e1 = sb.colStart[p + 1];
    for (int e = sb.colStart[p]; e < e1; ++e) {
      const ColumnSourceDev cs = sb.colSources[e];
      a += cs.weight * sourceGradientT(cs.joint, cs.dof, cs.parent, s.js, s.sub1 + kC1 * cs.tin);
    }
    thetaGrad[size_t(b) * P + p] = a;
  }
}

size_t stateBackwardLdsBytes(int J, int P) {
  return stateBackwardLdsFloats(J, P, nullptr, nullptr) * sizeof(float);
}

hipError_t launchStateBackward(
    const RigDev& rig, const StateBackwardDev& sb, int B, const float* theta, const float* stateGrad, float* thetaGrad, hipStream_t stream) {
  const size_t lds = stateBackwardLdsBytes(rig.J, rig.P);
  if (lds > 160 * 1024 - 64 || B <= 0) {
    return hipErrorInvalidValue;
  }
  static LdsLimitCache ldsLimit;
  hipError_t rc = ldsLimit.ensure(reinterpret_cast<const void*>(skeletonStateBackwardKernel), lds);
  if (rc != hipSuccess) {
    return rc;
  }
  hipLaunchKernelGGL(skeletonStateBackwardKernel, dim3(B), dim3(256), lds, stream, rig, sb, theta, stateGrad, thetaGrad);
  return hipGetLastError();
}

} // namespace mmx
