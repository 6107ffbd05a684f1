// mmx_wave.hip -- MMX_ROUTE_WAVE: the whole SolverT::solve loop with ONE WAVEFRONT per skeleton instance (gfx950, wave64).
//
// For small rigs (J <= MMX_WAVE_MAX_JOINTS, n <= MMX_WAVE_MAX_SOLVED): several instances per workgroup, each owned by one
// wave for the whole solve; no workgroup barrier anywhere (the waves of a workgroup leave the iteration loop at different
// iterations), the ordering of a wave's own LDS traffic is by waveSync().  What is computed is what fusedSolveKernel
// computes (mmx_fused.hip: GaussNewtonSolverT::doIteration inside SolverT::solve, the library's pivot / damping-floor /
// refinement / non-finite conventions); how it is computed differs:
//   A  forward kinematics: lanes = joints; the pointer-jumping rounds of fkJumpRoundsD with the partial products (double) in
//      REGISTERS, the ancestor's read by ds_bpermute -- the same products in the same order, no LDS buffer, no barrier
//   C  units: lanes = units (evalUnitFrom's L2 arithmetic)
//   G  H = J^T J, g = J^T r: the wave is split into 64 / NP groups of NP lanes (NP = 16 or 32: the padded system size); group
//      h, lane c holds column c of the three rows of unit u0 + h -- the entry gathered from the column's sources
//      (sourceDerivative) -- and that one register is both operands of v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32:
//      three matrix instructions per 2 / 4 units accumulate all of H; J is never stored
//   H  Cholesky with the rows in lanes (v_readlane broadcasts of the pivot column), kPivotFloor / kFactorDamping as everywhere
//   I  the two triangular solves, rows / columns of L in lanes
//   J  refinement through J: the rows are walked again, w = r - J d by a DPP reduction over the group's lanes, rho = J^T w - mu d
//   K  update: plain step or either backtracking rule (the last trial's joint states and units are the next iteration's)
// Per-wave LDS: theta, trial theta, joint states, unit vectors / residual rows / scales, the factor (NP x (NP + 4)):
// 9.5 KB for the 24-joint chain with position + orientation on every joint, 2.1 KB for a 3-joint character.
//
// Two translation units are built from this file.  Compiled as it is, it holds waveSolveKernel<16 / 32, false> behind
// launchWaveSolve (mmx_solve); mmx_wave_frames.hip includes it with MMX_WAVE_FRAMES_UNIT defined and then holds
// waveSolveKernel<16 / 32, true> behind launchWaveFrames (mmx_solve_frames) and nothing else.
#include <cfloat>

#include "mmx_kernels.hpp"

namespace mmx {

namespace {

typedef float wf32x16 __attribute__((ext_vector_type(16)));
typedef float wf32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaveThreads = 256; // four instances per workgroup

struct WaveCarve { // offsets in floats inside one wave's share of the workgroup's LDS (every one a multiple of 4)
  size_t th, tr, js, up, ur, us, utin, L, Linv, th0, total;
};
__host__ __device__ __forceinline__ size_t waveAlign4(size_t v) {
  return (v + 3) & ~size_t(3);
}
__host__ __device__ __forceinline__ WaveCarve waveCarve(int NP, int J, int P, int U, bool frames = false) {
  WaveCarve c;
  size_t p = 0;
  auto take = [&](size_t count) {
    const size_t r = p;
    p += waveAlign4(count);
    return r;
  };
  c.th = take(size_t(P));
  c.tr = take(size_t(P));
  c.js = take(size_t(kJs) * size_t(J));
  c.up = take(3 * size_t(U));
  c.ur = take(3 * size_t(U));
  c.us = take(size_t(U));
  c.utin = take(size_t(U));
  c.L = take(size_t(NP) * size_t(NP + 4));
  c.Linv = take(size_t(NP));
  c.th0 = frames ? take(size_t(P)) : 0; // (mmx_solve_frames: the parameters the wave's current frame started from)
  c.total = p;
  return c;
}

// What the kernel reads of the descriptors (RigDev / ProblemDev / FusedDev / SolveStateDev / FusedParams), gathered on the host.
// The kernel's ONLY parameter, so it sits at offset 0 of the kernarg segment: the kernel reads its fields through waveArgs(),
// a per-use opaque copy of the segment's address -- every field is then a scalar load next to its use instead of a scalar
// register held across the iteration loop (the descriptors by value: 360 spilled SGPRs in the 32-column instantiation).
struct WaveArgs {
  // rig
  int32_t J, P, jumpRounds, ptOffsetsNonZero;
  const int32_t* parent;
  const float* preRot; // shared [J][4], or [B][J][4] with instRig
  const float* offset; // shared [J][3], or [B][J][3] with instRig
  int32_t instPreRot, instOffset;
  const int4* ptEll;
  const int32_t* ptOuter;
  const int32_t* ptInner;
  const float* ptValue;
  const float* ptOffsets;
  // problem
  int32_t B, Kp, Ko, U, n, slotBase, fnCols, pad0;
  const int32_t* unitJoint;
  const int32_t* unitTin;
  const float* posOffset;
  const float* posTarget;
  const float* posWeight;
  const float* oriOffset;
  const float* oriTarget;
  const float* oriWeight;
  const float* fnWeights;
  float wPos, wOri, icPos, icOri;
  const ColumnSourceDev* srcs;
  const int32_t* srcStart;
  const int32_t* solveList;
  // solve
  float* theta;
  int32_t* iterations;
  int32_t* status;
  double* finalError;
  double* errorHistory;
  float* paramHistory;
  float lambda, threshold;
  int32_t minIterations, maxIterations, refine, doLineSearch;
  // frame sequences (waveSolveKernel<NP, true>): S sequences of F frames, instance f S + s = frame f of sequence s
  int32_t S, F;
};
typedef const __attribute__((address_space(4))) WaveArgs* WaveArgsPtr;
__device__ __forceinline__ WaveArgsPtr waveArgs() {
  WaveArgsPtr p = (WaveArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// orders a wave's own LDS traffic (writes by some lanes, reads by others): the hardware executes a wave's LDS instructions
// in order, the fences keep the compiler from moving them across
__device__ __forceinline__ void waveSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double shflD(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_ds_bpermute(src << 2, int(b));
  const int hi = __builtin_amdgcn_ds_bpermute(src << 2, int(b >> 32));
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<long long>(static_cast<unsigned int>(lo)));
}
__device__ __forceinline__ float shflF(float v, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
}

// lane kSel of v takes the uniform value `bits`; the other lanes keep theirs
template <int kSel>
__device__ __forceinline__ float writeLaneF(float v, int bits) {
  asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(bits), "n"(kSel));
  return v;
}

// sum over the lanes of a group of kW (16 or 32) consecutive lanes, the same value in every lane of the group (every step
// adds two values that the partner lane adds in the other order: commutative, hence identical)
template <int kW>
__device__ __forceinline__ double groupSumD(double v) {
  v += dppMoveD<0xB1>(v);
  v += dppMoveD<0x4E>(v);
  v += dppMoveD<0x141>(v);
  v += dppMoveD<0x140>(v);
  if (kW == 32) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_swizzle(int(b), 0x401F), hi = __builtin_amdgcn_ds_swizzle(int(b >> 32), 0x401F); // lane ^ 16
    v += __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<long long>(static_cast<unsigned int>(lo)));
  }
  return v;
}

// Forward kinematics of `th` (this wave's LDS) into js: lanes = joints.  Joint parameters (the transform's rows of the lane's
// joint: the same products in the same order as blockFk's walk), local transforms, the rounds of fkJumpRoundsD in registers,
// rotation axes.  th must be settled (waveSync) before; js is settled after.
__device__ __forceinline__ void waveFk(int b, const float* th, float* js, int lane) {
  const WaveArgsPtr A = waveArgs();
  const int J = A->J;
  const bool act = lane < J;
  const int j = act ? lane : 0;
  float jpv[7];
  const int4* ell = A->ptEll;
  const float* ptOffsets = A->ptOffsetsNonZero != 0 ? A->ptOffsets : nullptr;
  if (ell != nullptr) {
    int4 rows[7];
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      rows[d] = asGlobal(ell)[7 * j + d];
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      const int4 e = rows[d];
      float acc = 0.f;
      if (e.x >= 0) {
        acc += __int_as_float(e.y) * th[e.x];
      }
      if (e.z >= 0) {
        acc += __int_as_float(e.w) * th[e.z];
      }
      jpv[d] = acc + (ptOffsets != nullptr ? asGlobal(ptOffsets)[7 * j + d] : 0.f);
    }
  } else {
    const int32_t* ptOuter = A->ptOuter;
    const int32_t* ptInner = A->ptInner;
    const float* ptValue = A->ptValue;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      const int r = 7 * j + d;
      float acc = 0.f;
      const int k1 = asGlobal(ptOuter)[r + 1];
      for (int k = asGlobal(ptOuter)[r]; k < k1; ++k) {
        acc += asGlobal(ptValue)[k] * th[asGlobal(ptInner)[k]];
      }
      jpv[d] = acc + (ptOffsets != nullptr ? asGlobal(ptOffsets)[r] : 0.f);
    }
  }
  // the element's view of the rig (selectInstanceRig)
  const float* preRot = A->preRot + (A->instPreRot != 0 ? size_t(b) * 4 * size_t(J) : size_t(0));
  const float* offset = A->offset + (A->instOffset != 0 ? size_t(b) * 3 * size_t(J) : size_t(0));
  float pre[4], off3[3];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    pre[d] = asGlobal(preRot)[4 * j + d];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    off3[d] = asGlobal(offset)[3 * j + d];
  }
  const int par = asGlobal(A->parent)[j];
  const int rounds = A->jumpRounds;
  float loc[8], oq[8];
  fkLocalFromParams(jpv, pre, off3, loc, oq);
  float* slot = js + kJs * j;
  if (act) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      slot[8 + c] = oq[c];
    }
  }
  FkXf x;
  x.tx = loc[0], x.ty = loc[1], x.tz = loc[2], x.qx = loc[3], x.qy = loc[4], x.qz = loc[5], x.qw = loc[6], x.s = loc[7];
  x.jl = act ? par + 1 : 0;
  for (int r = 0; r < rounds; ++r) { // every lane reads the state its ancestor had at the START of the round
    const int a = x.jl - 1;
    const int src = a >= 0 ? a : lane;
    FkXf p;
    p.tx = shflD(x.tx, src), p.ty = shflD(x.ty, src), p.tz = shflD(x.tz, src);
    p.qx = shflD(x.qx, src), p.qy = shflD(x.qy, src), p.qz = shflD(x.qz, src), p.qw = shflD(x.qw, src);
    p.s = shflD(x.s, src);
    p.jl = __builtin_amdgcn_ds_bpermute(src << 2, x.jl);
    if (a >= 0) {
      fkComposeD(p, x);
    }
  }
  if (act) {
    slot[0] = float(x.tx), slot[1] = float(x.ty), slot[2] = float(x.tz);
    slot[3] = float(x.qx), slot[4] = float(x.qy), slot[5] = float(x.qz), slot[6] = float(x.qw);
    slot[7] = float(x.s);
  }
  waveSync();
  if (act) {
    fkAxesInPlaceQ(pre, j, par, js);
  }
  waveSync();
}

// Units from the joint states (lanes = units): loadUnitInput's reads and evalUnitFrom's arithmetic for the L2 loss, the
// element's function weights folded into the block weights (selectInstanceWeights).  Stores the unit vectors, the residual
// rows r = sigma f and sigma; returns the wave's error sum (uniform).
__device__ __forceinline__ double waveUnits(int b, const float* js, float* up, float* ur, float* us, int lane) {
  const WaveArgsPtr A = waveArgs();
  const int U = A->U, Kp = A->Kp, Ko = A->Ko;
  float wPos = A->wPos, wOri = A->wOri;
  const float icPos = A->icPos, icOri = A->icOri;
  const float* fnw = A->fnWeights;
  if (fnw != nullptr) {
    const int fnCols = A->fnCols;
    const float* w = asGlobal(fnw) + size_t(b) * size_t(fnCols);
    wPos *= fnCols > 0 ? w[0] : 1.f;
    wOri *= fnCols > 1 ? w[1] : 1.f;
  }
  const int32_t* unitJoint = A->unitJoint;
  const float* posOffset = A->posOffset;
  const float* posTarget = A->posTarget;
  const float* posWeight = A->posWeight;
  const float* oriOffset = A->oriOffset;
  const float* oriTarget = A->oriTarget;
  const float* oriWeight = A->oriWeight;
  double e = 0.0;
  for (int u = lane; u < U; u += 64) {
    const float* w = js + kJs * asGlobal(unitJoint)[u];
    const F3 t{w[0], w[1], w[2]};
    const Q4 q{w[3], w[4], w[5], w[6]};
    F3 v, f;
    float fw, ic, cw;
    if (u < Kp) { // position_error_function.cpp:23-26
      const size_t c = size_t(b) * Kp + u;
      const float* po = asGlobal(posOffset) + 3 * c;
      const float* pt = asGlobal(posTarget) + 3 * c;
      v = t + qrot(q, w[7] * F3{po[0], po[1], po[2]});
      f = v - F3{pt[0], pt[1], pt[2]};
      cw = asGlobal(posWeight)[c];
      fw = wPos, ic = icPos;
    } else { // orientation_error_function.cpp:23-39
      const int uo = u - Kp;
      const int co = uo / 3;
      const int k = uo - 3 * co;
      const size_t c = size_t(b) * Ko + co;
      const float* oo = asGlobal(oriOffset) + 4 * c;
      const float* ot = asGlobal(oriTarget) + 4 * c;
      const Q4 qo = qnormalized(Q4{oo[0], oo[1], oo[2], oo[3]});
      const Q4 qt = qnormalized(Q4{ot[0], ot[1], ot[2], ot[3]});
      v = qrot(q, qmatCol(qo, k));
      f = v - qmatCol(qt, k);
      cw = asGlobal(oriWeight)[c];
      fw = wOri, ic = icOri;
    }
    float sigma = 0.f, werr = 0.f;
    if (cw != 0.f && fw > 0.f) { // joint_error_function-inl.h:197-213
      const float wgt = cw * fw;
      werr = wgt * (dot(f, f) * ic);
      sigma = sqrtf(wgt * ic);
    }
    up[3 * u] = v.x, up[3 * u + 1] = v.y, up[3 * u + 2] = v.z;
    ur[3 * u] = sigma * f.x, ur[3 * u + 1] = sigma * f.y, ur[3 * u + 2] = sigma * f.z;
    us[u] = sigma;
    e += double(werr);
  }
  e = waveReduceSum(e);
  waveSync();
  return e;
}

// d(unit vector) / d(solved parameter of this lane): the column's primary source (registers) and its further ones
__device__ __forceinline__ F3 waveColumnDerivative(const ColumnSourceDev& s0, const ColumnSourceDev* srcs, int x0, int x1, const float* js, const Unit& un) {
  F3 dv{0.f, 0.f, 0.f};
  bool ap;
  const F3 d0 = sourceDerivative(s0, js, un, ap);
  if (ap) {
    dv = s0.weight * d0;
  }
  for (int e = x0; e < x1; ++e) {
    const ColumnSourceDev s = asGlobal(srcs)[e];
    const F3 d = sourceDerivative(s, js, un, ap);
    if (ap) {
      dv = dv + s.weight * d;
    }
  }
  return dv;
}

template <int NP>
struct WaveAcc;
template <>
struct WaveAcc<32> {
  wf32x16 v;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      v[i] = 0.f;
    }
  }
  __device__ __forceinline__ void add(float a) { v = __builtin_amdgcn_mfma_f32_32x32x2f32(a, a, v, 0, 0, 0); }
  // D[row][col]: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  __device__ __forceinline__ void store(float* L, int lane) const {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      L[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 36 + (lane & 31)] = v[r];
    }
  }
};
template <>
struct WaveAcc<16> {
  wf32x4 v;
  __device__ __forceinline__ void zero() { v[0] = v[1] = v[2] = v[3] = 0.f; }
  __device__ __forceinline__ void add(float a) { v = __builtin_amdgcn_mfma_f32_16x16x4f32(a, a, v, 0, 0, 0); }
  // col = lane & 15, row = 4 (lane >> 4) + reg
  __device__ __forceinline__ void store(float* L, int lane) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      L[(4 * (lane >> 4) + r) * 20 + (lane & 15)] = v[r];
    }
  }
};

// Elimination step j (and the ones after it) of the Cholesky with the rows in lanes: lane j's a[j] is the pivot d_jj -- at or
// below its floor the column is dropped (see kPivotFloor) --, kept in lane j of rawPivot, 1 / l_jj in lane j of invd
// (v_writelane: no lane mask and no branch in the chain -- either one per step costs an SGPR pair held across the chain)
template <int NP, int j>
__device__ __forceinline__ void waveFactorStep(float (&a)[NP], float floorRow, float& rawPivot, float& invd) {
  const float pv = a[j] > floorRow ? __builtin_amdgcn_rsqf(a[j]) : 0.f;
  rawPivot = writeLaneF<j>(rawPivot, __builtin_amdgcn_readlane(__float_as_int(a[j]), j));
  const int invBits = __builtin_amdgcn_readlane(__float_as_int(pv), j);
  invd = writeLaneF<j>(invd, invBits);
  a[j] *= __int_as_float(invBits);
#pragma unroll
  for (int k = j + 1; k < NP; ++k) {
    a[k] -= a[j] * readLaneF(a[j], k);
  }
  if constexpr (j + 1 < NP) {
    waveFactorStep<NP, j + 1>(a, floorRow, rawPivot, invd);
  }
}

// L L^T x = rhs with lane i holding entry i of rhs (lanes >= NP: their column's, unused).  The factor in LDS holds l_ij below
// the diagonal, ZEROS on and above it, and 1 / l_ii in Linv (0: the column was dropped); the rows of L (forward) and its
// columns (backward) are read into the lane.  A lane's running value stops changing once its own unknown is reached (the
// entries at and beyond it are zero), so no step needs a lane mask.  Returns x_i in every lane of column i.
template <int NP>
__device__ __forceinline__ float waveSolveLLt(const float* L, const float* Linv, float rhs, int lane) {
  constexpr int LS = NP + 4;
  int i = lane & (NP - 1);
  asm volatile("" : "+v"(i)); // (nothing derived from the lane index is to be hoisted out of the iteration loop)
  float a[NP];
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    a[c] = L[i * LS + c];
  }
  const float invd = Linv[i];
  float bi = rhs;
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    bi -= a[c] * readLaneF(bi * invd, c);
  }
  bi *= invd;
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    a[c] = L[c * LS + i];
  }
#pragma unroll
  for (int c = NP - 1; c >= 0; --c) {
    bi -= a[c] * readLaneF(bi * invd, c);
  }
  return bi * invd;
}

// kFrames (mmx_solve_frames): the wave owns SEQUENCE s = the instances s, S + s, 2 S + s, ... and solves them one after the
// other, each from the result of the one before -- theta stays in the wave's LDS, the problem-shared tables (the column's
// sources, solveIdx, utin) are loaded once, everything an instance's solve carries is reset per frame.
template <int NP, bool kFrames>
__global__ void __launch_bounds__(kWaveThreads) waveSolveKernel(const WaveArgs argsInKernargSegment) {
  (void)argsInKernargSegment; // read through waveArgs()
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int G = 64 / NP; // units per matrix instruction triple
  constexpr int LS = NP + 4; // row stride of the factor in LDS
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  int b = int(blockIdx.x) * (kWaveThreads / 64) + wave; // (kFrames: the sequence = its frame 0; moves on by S per frame)
  if (b >= (kFrames ? waveArgs()->S : waveArgs()->B)) {
    return; // (no workgroup barrier anywhere below)
  }
  int P, U, n, Kp;
  float *th, *tr, *js, *up, *ur, *us, *Ls, *Linv;
  [[maybe_unused]] float* th0 = nullptr; // kFrames: the frame's initial parameters
  int* utin;
  // this lane's column of the system: group h = lane / NP, column c = lane % NP
  const int c = lane & (NP - 1), h = lane / NP;
  ColumnSourceDev s0{0, 3, 0, 0, -1, 0.f}; // (a source that applies to no unit)
  int x0 = 0, x1 = 0, solveIdx = 0;
  {
    const WaveArgsPtr A = waveArgs();
    P = A->P, U = A->U, n = A->n, Kp = A->Kp;
    __builtin_assume(U > 0 && n > 0 && P > 0); // (launchWaveSolve refuses anything else)
    const WaveCarve cv = waveCarve(NP, A->J, P, U, kFrames);
    float* base = smem + size_t(wave) * cv.total;
    th = base + cv.th, tr = base + cv.tr, js = base + cv.js, up = base + cv.up, ur = base + cv.ur, us = base + cv.us;
    utin = reinterpret_cast<int*>(base + cv.utin);
    Ls = base + cv.L, Linv = base + cv.Linv;
    // (the wave's LDS addresses live in VECTOR registers from here on: uniform, but nine more scalar registers -- and everything
    // the compiler derives from them ahead of the loop -- are what spilled)
    asm volatile("" : "+v"(th), "+v"(tr), "+v"(js), "+v"(up), "+v"(ur), "+v"(us), "+v"(utin), "+v"(Ls), "+v"(Linv));
    const float* thg = A->theta + size_t(b) * P;
    if constexpr (kFrames) {
      th0 = base + cv.th0;
      asm volatile("" : "+v"(th0));
      for (int i = lane; i < P; i += 64) {
        th[i] = th0[i] = thg[i];
      }
    } else {
      for (int i = lane; i < P; i += 64) {
        th[i] = thg[i];
      }
    }
    const int32_t* unitTin = A->unitTin;
    for (int u = lane; u < U; u += 64) {
      utin[u] = asGlobal(unitTin)[u];
    }
    if (c < n) {
      s0 = asGlobal(A->srcs)[c];
      x0 = A->slotBase + asGlobal(A->srcStart)[c];
      x1 = A->slotBase + asGlobal(A->srcStart)[c + 1];
      solveIdx = asGlobal(A->solveList)[c];
    }
  }
  waveSync();
  const int laneO = lane;
  const ColumnSourceDev s0O = s0;

  // one pass = one instance's solve; kFrames: a pass per frame, everything below the loop head is per-frame state (above all
  // stateValid: the joint states and units a line search left in LDS are the PREVIOUS frame's payload's)
  for ([[maybe_unused]] int frame = 0;;) {
    double lastError = DBL_MAX; // solver.cpp:84-85
    double curError = DBL_MAX;
    int itersDone = 0, status = 0;
    bool stateValid = false; // js / up / ur / us already belong to th (left by the last trial of a line search)
    double stateError = 0.0;

    for (int it = 0; it < waveArgs()->maxIterations; ++it) {
      // Opaque per-iteration copies of the lane index and of the lane's primary source: what derives from them (lane masks of the
      // dof tests, addresses) is recomputed where it is used instead of being held in scalar registers across the iteration loop
      int lane = laneO;
      asm volatile("" : "+v"(lane));
      const int c = lane & (NP - 1), h = lane / NP;
      const bool colLive = c < n;
      ColumnSourceDev s0 = s0O;
      asm volatile("" : "+v"(s0.joint), "+v"(s0.dof), "+v"(s0.tin), "+v"(s0.tout), "+v"(s0.parent), "+v"(s0.weight));
      // the lane's unit of the group round starting at u0 (a unit beyond U: tin -1 and sigma 0 -- no source applies)
      auto unitAt = [&](int u0, Unit& un, float& sigma, int& ui) {
        const int u = u0 + h;
        ui = u < U ? u : U - 1;
        un.v = F3{up[3 * ui], up[3 * ui + 1], up[3 * ui + 2]};
        un.isPoint = ui < Kp;
        un.tin = u < U ? utin[ui] : -1;
        sigma = u < U ? us[ui] : 0.f;
      };
      // total of a per-lane partial over the groups, for the lane's column (the same order in every lane of a column)
      auto overGroups = [&](float part) {
        float tot = 0.f;
    #pragma unroll
        for (int k = 0; k < G; ++k) {
          tot += shflF(part, c + k * NP);
        }
        return tot;
      };
      // ================= A-C
      if (stateValid) {
        curError = stateError;
      } else {
        waveFk(b, th, js, lane);
        curError = waveUnits(b, js, up, ur, us, lane);
      }
      const float lambda = waveArgs()->lambda;
      // ================= G: H = J^T J on the matrix cores, g = J^T r
      float gc;
      {
        const ColumnSourceDev* srcs = waveArgs()->srcs;
        WaveAcc<NP> acc;
        acc.zero();
        float gpart = 0.f;
        for (int u0 = 0; u0 < U; u0 += G) {
          Unit un;
          float sigma;
          int ui;
          unitAt(u0, un, sigma, ui);
          const F3 dv = waveColumnDerivative(s0, srcs, x0, x1, js, un);
          const float jx = sigma * dv.x, jy = sigma * dv.y, jz = sigma * dv.z;
          acc.add(jx);
          acc.add(jy);
          acc.add(jz);
          gpart += jx * ur[3 * ui] + jy * ur[3 * ui + 1] + jz * ur[3 * ui + 2];
        }
        gc = overGroups(gpart);
        acc.store(Ls, lane);
      }
      waveSync();
      // ================= H: damping (gauss_newton_solver.cpp:248) with the factor's floor (kFactorDamping), Cholesky with the
      // rows in lanes; the factor goes back to LDS strictly lower triangular, 1 / l_ii beside it
      bool badPivot = false, floored = false;
      {
        int i = c; // (the groups beyond the first factor redundantly)
        asm volatile("" : "+v"(i)); // (nothing derived from the lane index is to be hoisted out of the iteration loop)
        const float hii = Ls[i * LS + i];
        const float trace = waveReduceSumF(lane < n ? hii : 0.f);
        const float muFactor = fmaxf(lambda, kFactorDamping * trace / float(n > 0 ? n : 1));
        floored = muFactor > lambda;
        const float hd = i < n ? hii + muFactor : 1.f; // padded rows / columns form an identity block
        const float floorRow = kPivotFloor * hd;
        waveSync();
        if (lane < NP) {
          Ls[i * LS + i] = hd;
        }
        waveSync();
        float a[NP];
  #pragma unroll
        for (int k = 0; k < NP; ++k) {
          a[k] = Ls[i * LS + k];
        }
        waveSync(); // every lane holds its row before the factor overwrites H
        float rawPivot = 1.f, invd = 0.f; // lane j: d_jj as it came out, 1 / l_jj
        waveFactorStep<NP, 0>(a, floorRow, rawPivot, invd);
        badPivot = __builtin_amdgcn_ballot_w64(!(rawPivot > 0.f)) != 0ull;
        // back to LDS: the rows as they are, then every lane clears its row from the diagonal on (a loop over addresses, not 32
        // lane masks: those cost an SGPR pair each)
        if (lane < NP) {
  #pragma unroll
          for (int k = 0; k < NP; ++k) {
            Ls[i * LS + k] = a[k];
          }
          Linv[i] = invd;
        }
        waveSync();
        if (lane < NP) {
          for (int k = i; k < NP; ++k) {
            Ls[i * LS + k] = 0.f;
          }
        }
      }
      waveSync();
      // ================= I: the step (every lane of column c holds d_c)
      float dc = waveSolveLLt<NP>(Ls, Linv, colLive ? gc : 0.f, lane);
      // ================= J: refinement through J (the rule of fusedSolveKernel phase J)
      {
        const int refine = waveArgs()->refine;
        float prevCorr2 = FLT_MAX;
        for (int rf = 0; rf < refine; ++rf) {
          const ColumnSourceDev* srcs = waveArgs()->srcs;
          // The two products of the residual are carried in DOUBLE (the entries of J stay the single-precision ones): a problem with
          // fewer rows than parameters (BASELINE configs[0]: 9 rows, 31 parameters) amplifies the rounding of rho by 1 / lambda in
          // the directions J does not determine -- in single precision the committed fixture sat at 1.9e-4 of the double oracle,
          // the bound being 5e-5
          double rpart = 0.0;
          for (int u0 = 0; u0 < U; u0 += G) {
            Unit un;
            float sigma;
            int ui;
            unitAt(u0, un, sigma, ui);
            const F3 dv = waveColumnDerivative(s0, srcs, x0, x1, js, un);
            // w = r - J d for the unit's three rows; y = sigma w
            const double dd = double(dc), sg = double(sigma);
            const double sx = groupSumD<NP>(dd * double(dv.x)), sy = groupSumD<NP>(dd * double(dv.y)), sz = groupSumD<NP>(dd * double(dv.z));
            const double yx = sg * (double(ur[3 * ui]) - sg * sx), yy = sg * (double(ur[3 * ui + 1]) - sg * sy), yz = sg * (double(ur[3 * ui + 2]) - sg * sz);
            rpart += double(dv.x) * yx + double(dv.y) * yy + double(dv.z) * yz;
          }
          double jtw = 0.0;
  #pragma unroll
          for (int k = 0; k < G; ++k) {
            jtw += shflD(rpart, c + k * NP);
          }
          const float cr = waveSolveLLt<NP>(Ls, Linv, colLive ? float(jtw - double(lambda) * double(dc)) : 0.f, lane);
          const float dn = dc + cr;
          const bool mine = lane < n;
          const float corr2 = waveReduceSumF(mine ? cr * cr : 0.f);
          const float step2 = waveReduceSumF(mine ? dn * dn : 0.f);
          if (refineUndo(corr2, step2, prevCorr2)) { // not a contraction
            dc = dn - cr;
            break;
          }
          dc = dn;
          prevCorr2 = corr2;
          if (!refineAgain(corr2, step2)) {
            break;
          }
        }
      }
      // ================= K: update (gauss_newton_solver.cpp:283-313, gauss_newton_solver_qr.cpp:126-149)
      const int doLineSearch = waveArgs()->doLineSearch;
      if (doLineSearch != MMX_LINE_SEARCH_NONE) {
        const float scaledError = 1e-3f * float(curError);
        double gd = 0.0;
        if (doLineSearch == MMX_LINE_SEARCH_DIRECTIONAL) {
          gd = double(waveReduceSumF(lane < n ? gc * dc : 0.f));
        }
        float scale = 1.f;
        for (int ls = 0; ls < 10; ++ls) {
          for (int i = lane; i < P; i += 64) {
            tr[i] = th[i];
          }
          waveSync();
          if (lane < n) {
            tr[solveIdx] -= scale * dc;
          }
          waveSync();
          waveFk(b, tr, js, lane);
          stateError = waveUnits(b, js, up, ur, us, lane);
          if (armijoAccepts(doLineSearch, curError, stateError, scale, scaledError, gd)) {
            break;
          }
          scale *= 0.5f;
        }
        for (int i = lane; i < P; i += 64) {
          th[i] = tr[i];
        }
        stateValid = true; // the last trial evaluated IS the new theta
      } else {
        if (lane < n) {
          th[solveIdx] -= dc; // skeleton_solver_function.cpp:158
        }
      }
      waveSync();
      {
        const WaveArgsPtr A = waveArgs();
        const size_t row = size_t(b) * A->maxIterations + it;
        float* paramHistory = A->paramHistory;
        if (paramHistory != nullptr) { // solver.cpp:101-106
          float* ph = asGlobal(paramHistory) + row * size_t(P);
          for (int i = lane; i < P; i += 64) {
            ph[i] = th[i];
          }
        }
        double* errorHistory = A->errorHistory;
        if (errorHistory != nullptr && lane == 0) {
          asGlobal(errorHistory)[row] = curError;
        }
        itersDone = it + 1;
        status |= badPivot ? MMX_SOLVE_NOT_PD : 0;
        status |= floored ? MMX_SOLVE_DAMPING_FLOORED : 0;
        const bool stop = solveStops(it, A->minIterations, lastError, curError, A->threshold);
        lastError = curError;
        asm volatile("" : "+v"(lastError)); // (kept in vector registers across the iteration: two scalar registers fewer)
        if (stop) {
          break;
        }
      }
    }

    // NaN / Inf guard of the batched driver: theta in global memory still holds the initial parameters, "revert" = do not write
    int laneE = laneO; // (an opaque copy: the loop masks below are not the prologue's, held across the whole solve)
    asm volatile("" : "+v"(laneE));
    int bad = 0;
    for (int i = laneE; i < P; i += 64) {
      bad |= isfinite(th[i]) ? 0 : 1;
    }
    const bool anyBad = __builtin_amdgcn_ballot_w64(bad != 0) != 0ull;
    const WaveArgsPtr A = waveArgs();
    if constexpr (kFrames) {
      // the frame's row takes its result -- or, reverted, the parameters it started from --, and that is where the next frame starts
      // (each lane keeps to its own entries of th / th0: no ordering needed among the three)
      float* thg = asGlobal(A->theta) + size_t(b) * P;
      for (int i = laneE; i < P; i += 64) {
        const float v = anyBad ? th0[i] : th[i];
        th[i] = v, th0[i] = v, thg[i] = v;
      }
    } else if (!anyBad) {
      float* thg = asGlobal(A->theta) + size_t(b) * P;
      for (int i = laneE; i < P; i += 64) {
        thg[i] = th[i];
      }
    }
    if (laneE == 0) {
      asGlobal(A->iterations)[b] = itersDone;
      asGlobal(A->finalError)[b] = curError;
      asGlobal(A->status)[b] = solveStatus(anyBad, status);
    }
    if constexpr (kFrames) {
      if (++frame >= A->F) {
        break;
      }
      b += A->S;
      waveSync(); // th is settled before the next frame's forward kinematics reads it
    } else {
      break;
    }
  }
}

template <int NP, bool kFrames>
hipError_t launchWaveNP(const WaveArgs& a, size_t lds, hipStream_t stream) {
  static LdsLimitCache ldsLimit; // (one per instantiation)
  hipError_t rc = ldsLimit.ensure(reinterpret_cast<const void*>(waveSolveKernel<NP, kFrames>), lds);
  if (rc != hipSuccess) {
    return rc;
  }
  const int perGroup = kWaveThreads / 64;
  const int waves = kFrames ? a.S : a.B;
  hipLaunchKernelGGL((waveSolveKernel<NP, kFrames>), dim3((waves + perGroup - 1) / perGroup), dim3(kWaveThreads), lds, stream, a);
  return hipGetLastError();
}

// numFrames 0: one wave per instance (mmx_solve); >= 1: one wave per sequence of numFrames frames (mmx_solve_frames)
template <bool kFrames>
hipError_t launchWave(const RigDev& rig, const ProblemDev& pb, const FusedDev& fd, float* theta, const SolveStateDev& st, const FusedParams& fp, int numFrames, hipStream_t stream) {
  constexpr bool frames = kFrames;
  const size_t lds = waveLdsBytes(rig.J, rig.P, fd.U, fd.n, frames);
  if (rig.J > MMX_WAVE_MAX_JOINTS || fd.n > MMX_WAVE_MAX_SOLVED || fd.n <= 0 || fd.U <= 0 || fd.U > MMX_WAVE_MAX_UNITS || lds > 160 * 1024 ||
      pb.lossPos.type != 0 || pb.lossOri.type != 0 || pb.instPosParent != nullptr || pb.instOriParent != nullptr ||
      (frames && (pb.B <= 0 || pb.B % numFrames != 0))) {
    return hipErrorInvalidValue;
  }
  WaveArgs a{};
  a.J = rig.J, a.P = rig.P, a.jumpRounds = rig.jumpRounds, a.ptOffsetsNonZero = rig.ptOffsetsNonZero;
  a.parent = rig.parent;
  a.preRot = rig.instPreRot != nullptr ? rig.instPreRot : rig.preRot;
  a.offset = rig.instOffset != nullptr ? rig.instOffset : rig.offset;
  a.instPreRot = rig.instPreRot != nullptr ? 1 : 0;
  a.instOffset = rig.instOffset != nullptr ? 1 : 0;
  a.ptEll = rig.ptEll, a.ptOuter = rig.ptOuter, a.ptInner = rig.ptInner, a.ptValue = rig.ptValue, a.ptOffsets = rig.ptOffsets;
  a.B = pb.B, a.Kp = pb.Kp, a.Ko = pb.Ko, a.U = fd.U, a.n = fd.n, a.slotBase = fd.slotBase, a.fnCols = pb.fnCols;
  a.unitJoint = pb.unitJoint, a.unitTin = pb.unitTin;
  a.posOffset = pb.posOffset, a.posTarget = pb.posTarget, a.posWeight = pb.posWeight;
  a.oriOffset = pb.oriOffset, a.oriTarget = pb.oriTarget, a.oriWeight = pb.oriWeight;
  a.fnWeights = pb.fnWeights;
  a.wPos = pb.wPos, a.wOri = pb.wOri, a.icPos = pb.lossPos.invC2, a.icOri = pb.lossOri.invC2;
  a.srcs = fd.srcs, a.srcStart = fd.srcStart, a.solveList = fd.solveList;
  a.theta = theta;
  a.iterations = st.iterations, a.status = st.status, a.finalError = st.finalError;
  a.errorHistory = st.errorHistory, a.paramHistory = st.paramHistory;
  a.lambda = fp.lambda, a.threshold = fp.threshold;
  a.minIterations = fp.minIterations, a.maxIterations = fp.maxIterations, a.refine = fp.refine, a.doLineSearch = fp.doLineSearch;
  if constexpr (frames) {
    a.S = pb.B / numFrames, a.F = numFrames;
  }
  return fd.n <= 16 ? launchWaveNP<16, kFrames>(a, lds, stream) : launchWaveNP<32, kFrames>(a, lds, stream);
}

} // namespace

#ifndef MMX_WAVE_FRAMES_UNIT
size_t waveLdsBytes(int J, int P, int U, int n, bool frames) {
  return size_t(kWaveThreads / 64) * waveCarve(n <= 16 ? 16 : 32, J, P, U, frames).total * sizeof(float);
}

hipError_t launchWaveSolve(const RigDev& rig, const ProblemDev& pb, const FusedDev& fd, float* theta, const SolveStateDev& st, const FusedParams& fp, hipStream_t stream) {
  return launchWave<false>(rig, pb, fd, theta, st, fp, 0, stream);
}
#else
hipError_t launchWaveFrames(const RigDev& rig, const ProblemDev& pb, const FusedDev& fd, float* theta, const SolveStateDev& st, const FusedParams& fp, int numFrames, hipStream_t stream) {
  return numFrames > 0 ? launchWave<true>(rig, pb, fd, theta, st, fp, numFrames, stream) : hipErrorInvalidValue;
}
#endif

} // namespace mmx
