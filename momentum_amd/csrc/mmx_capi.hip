// mmx_capi.hip -- implementation of the C ABI declared in include/mmx.h.
// Host-side glue only: handle ownership, device buffers, table upload, kernel sequencing.
// No compute happens on the host and there is no CPU fallback: without a HIP device every compute
// entry point returns MMX_ERR_NO_DEVICE / MMX_ERR_DEVICE.
#include "../../include/mmx.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "mmx_constraint_intake.hpp"
#include "mmx_host_tables.hpp"
#include "mmx_kernels.hpp"
#include "mmx_skin_tables.hpp"
#include "mmx_solve_plan.hpp"
#include "mmx_vertex_constraints.hpp"
#include "mmx_skin_normal_equations_plan.hpp"

namespace {

thread_local std::string g_lastError;

int32_t fail(int32_t code, const std::string& msg) {
  g_lastError = msg;
  return code;
}

#define MMX_HIP(call)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      return fail(                                                                                \
          e_ == hipErrorOutOfMemory ? MMX_ERR_OUT_OF_MEMORY : MMX_ERR_DEVICE,                     \
          std::string(#call) + ": " + hipGetErrorString(e_));                                     \
    }                                                                                             \
  } while (0)

// ... and the same for a step that answers with a status code of its own
#define MMX_TRY(call)        \
  do {                       \
    int32_t rc_ = (call);    \
    if (rc_ != MMX_OK) {     \
      return rc_;            \
    }                        \
  } while (0)

// ---- profiling zones: roctx ranges around the ABI entry points and the phases of the explicit-Jacobian
// iteration, named after the reference's MT_PROFILE_EVENT zones of this path
// (momentum/solver/gauss_newton_solver.cpp:70,225,241,264,285,290; solver.cpp:51).  The roctx library is
// looked up at run time (librocprofiler-sdk-roctx.so, then libroctx64.so) so that libmmx_hip.so has no
// link-time dependency on a profiler; without it, or with MMX_NO_ROCTX set, a zone costs one branch.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (getenv("MMX_NO_ROCTX") != nullptr) {
      return;
    }
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      void* h = dlopen(name, RTLD_LAZY | RTLD_LOCAL);
      if (h != nullptr) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push != nullptr && pop != nullptr) {
          return;
        }
        push = nullptr, pop = nullptr;
      }
    }
  }
};
const Roctx& roctx() {
  static const Roctx r;
  return r;
}
struct Zone {
  bool open;
  explicit Zone(const char* name) : open(roctx().push != nullptr) {
    if (open) {
      roctx().push(name);
    }
  }
  Zone(const Zone&) = delete;
  Zone& operator=(const Zone&) = delete;
  ~Zone() {
    if (open) {
      roctx().pop();
    }
  }
};
#define MMX_ZONE_CAT2(a, b) a##b
#define MMX_ZONE_CAT(a, b) MMX_ZONE_CAT2(a, b)
#define MMX_ZONE(name) Zone MMX_ZONE_CAT(zone_, __LINE__)(name)

// RAII device buffer
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    release();
  }
  void release() {
    if (p != nullptr) {
      (void)hipFree(p);
      p = nullptr;
      bytes = 0;
    }
  }
  hipError_t ensure(size_t n) {
    if (n <= bytes && p != nullptr) {
      return hipSuccess;
    }
    release();
    if (n == 0) {
      return hipSuccess;
    }
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) {
      bytes = n;
    } else {
      p = nullptr;
    }
    return e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

template <class T>
hipError_t upload(DevBuf& buf, const std::vector<T>& v) {
  hipError_t e = buf.ensure(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (e != hipSuccess || v.empty()) {
    return e;
  }
  return hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// Brings the arrays a setter is handed (float or int32 payload, all of one memory kind) to the device: null or empty -> null;
// MMX_MEM_DEVICE -> the caller's pointer, borrowed; MMX_MEM_HOST -> copied into the handle's buffer ON THE CALLER'S STREAM, so
// ordered after the kernels in flight there that still read the previous payload (torch's streams do not wait for the null
// stream).  The host copies are complete -- the caller may free its arrays -- once finish() has returned; a setter that leaves
// early with an error waits in the destructor.
struct Staging {
  int32_t memory;
  hipStream_t stream;
  bool pending = false;
  Staging(int32_t memory_, hipStream_t stream_) : memory(memory_), stream(stream_) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() {
    (void)finish();
  }
  template <class T>
  hipError_t bring(DevBuf& buf, const T* src, size_t count, const T*& dst) {
    static_assert(sizeof(T) == 4, "float and int32 payloads");
    dst = nullptr;
    if (src == nullptr || count == 0) {
      return hipSuccess;
    }
    if (memory == MMX_MEM_DEVICE) {
      dst = src;
      return hipSuccess;
    }
    hipError_t e = buf.ensure(count * sizeof(T));
    if (e != hipSuccess) {
      return e;
    }
    dst = buf.as<T>();
    pending = true;
    return hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, stream);
  }
  hipError_t finish() {
    const bool wait = pending;
    pending = false;
    return wait ? hipStreamSynchronize(stream) : hipSuccess;
  }
};

} // namespace

namespace mmx {
int32_t failWith(int32_t code, const std::string& msg) { // for the other translation units of the C ABI
  return fail(code, msg);
}
} // namespace mmx

struct mmx_rig {
  int32_t device = 0;
  int32_t J = 0, P = 0;
  // host copy of the descriptor (needed to rebuild tables when the enabled set changes)
  std::vector<int32_t> parent, ptOuter, ptInner;
  std::vector<float> preRot, offset, ptValue, ptOffsets;
  mmx::HostTables topo; // built with all parameters enabled
  DevBuf dParent, dPreRot, dOffset, dPtOuter, dPtInner, dPtValue, dPtOffsets, dLevelOrder, dLevelStart, dPtEll, dJumpParent, dPtRowRec;
  mmx::RigDev dev{};
  // mmx_eval_skeleton_state_backward's tables (mmx::buildStateBackwardTables): built from `topo` and uploaded by the first
  // call on the rig, then kept -- they depend on the rig alone
  std::mutex sbMutex;
  bool sbReady = false;
  DevBuf dSbSubSize, dSbLoadedPos, dSbJointPos, dSbColStart, dSbColSources;
  mmx::StateBackwardDev sbDev{};

  mmx_rig_desc desc() const {
    mmx_rig_desc d{};
    d.num_joints = J;
    d.num_params = P;
    d.parent = parent.data();
    d.pre_rotation = preRot.data();
    d.translation_offset = offset.data();
    d.pt_outer = ptOuter.data();
    d.pt_inner = ptInner.data();
    d.pt_value = ptValue.data();
    d.pt_offsets = ptOffsets.data();
    return d;
  }
};

// A skin on a rig (mmx_skin_create): the uploaded tables of linear-blend skinning and the staging buffers of the _host forms
struct mmx_skin {
  mmx_rig* rig = nullptr;
  DevBuf dJoint, dWeight, dInverseBind, dRest, dJointStart, dEntryVertex, dEntryWeight, dWaveStart;
  mmx::SkinDev dev{};
  DevBuf sState, sRest, sOut, sStateGrad, sRestGrad;
  DevBuf sVcVertex, sVcBary, sVcTarget, sVcNormal, sVcWeight, sVcTheta, sVcJtj, sVcJtr, sVcErr; // mmx_skin_normal_equations_host
};

struct mmx_problem {
  mmx_rig* rig = nullptr;
  int32_t B = 0, Kp = 0, Ko = 0, U = 0, M = 0;
  std::vector<int32_t> posParent, oriParent;
  // per-instance characters / constraint parents (mmx_problem_set_instance_rig / _parents)
  mmx::RigDev rigDev{}; // the rig as this problem's kernels see it: rig->dev + the per-instance pointers
  DevBuf oInstOffset, oInstPreRot, oInstPosParent, oInstOriParent, dJointTin;
  std::vector<int32_t> unionPos, unionOri; // joints that carry a position / orientation constraint in some element
  std::vector<int32_t> instPosHost, instOriHost; // the lists of the last mmx_problem_set_instance_parents call (host copies)
  bool instParentsFromHost = false;
  bool instPos = false, instOri = false;
  mmx::HostTables tables; // for the current enabled set
  mmx::FusedTables fused;
  DevBuf dUnitJoint, dUnitTin, dColStart, dColSources, dEnabledList, dJacRecs, dMultiCols, dZeroCols;
  DevBuf dSubSize, dPosUnitStart, dPosUnits, dSolveList, dSrcStart, dSrcs, dTerms, dTerms16, dComb, dDfsJoint, dLoadedPos;
  DevBuf dLimStart, dLimOf, dPairDest, dPairStart, dPairLim, dPairCols;
  mmx::FusedDev fdev{};
  // constraint payload: owned copies (host ingest) or borrowed device pointers
  DevBuf oPosOffset, oPosTarget, oPosWeight, oOriOffset, oOriTarget, oOriWeight, oMpTarget, oMpWeights, dLimits, dEnabledMask, oFnWeights;
  std::vector<mmx_parameter_limit> limits; // host copy (solve-list bookkeeping)
  // further joint-constraint blocks: their topology (host copy) and, per block, the owned copies of a host payload
  std::vector<mmx::ProblemTopology::Block> blocks;
  struct BlockPayload {
    DevBuf oLocalPoint, oLocalDir, oGlobal, oPlaneD, oWeight, oProjection;
  };
  std::vector<std::unique_ptr<BlockPayload>> blockPayload; // [blocks.size()]
  std::vector<mmx::JointBlockDev> blockDev;
  std::vector<mmx_ellipsoid_limit> ellipsoids; // host copy
  DevBuf dEllipsoids;
  DevBuf dBlocks, dGenJoint, dGenTin, dGenBlock;
  int32_t genRows = 0;
  bool haveConstraints = false;
  bool tablesDirty = false; // blocks / ellipsoids / limits changed and uploadProblemTables has not succeeded since
  mmx::ProblemDev dev{};
  // the same problem with the structurally zero columns dropped from the solve (explicit-Jacobian solver)
  int32_t solveN = 0;
  DevBuf dSolveListV1; // [solveN]
  DevBuf sHess2F64; // mmx_solve_f64 under MMX_STEP_TRUST_REGION: J^T J without damping
  DevBuf dSolveListF64; // [solveN] the same parameters in index order: the double instantiation follows the reference's column order
  std::vector<int32_t> solveListF64;
  std::vector<std::pair<int32_t, int32_t>> limitPairs; // (row, col) solve columns of the off-diagonal H entries limits add
  DevBuf dTileMasks, dTileList; // tile structure of the factor in elimination order (mmx::TileMasks): [64] masks, the non-zero tiles
  mmx::TileMasks tileMasks;
  std::vector<int32_t> solveListV1; // host copy
  // scratch
  DevBuf sJac, sRes, sErr, sJtj, sJtr, sFactor, sThetaInit, sTheta;
  DevBuf sTreeState, sDvec, sRhoVec, sRefState, sGenState; // wide systems refined through the tree (no dense J)
  DevBuf sJacColMajor; // column-major J of an MMX_LAYOUT_ROW_MAJOR request, before its transposition
  DevBuf sJacF64, sHessF64; // scratch of the double-precision solve
  // mmx_solve_f64's assembly list (mmx::F64AssemblyList): built on first use for the launch's chunking, dropped when the
  // tables change (uploadProblemTables)
  DevBuf dF64Groups, dF64Extra, dF64ChunkStart;
  int32_t f64ListUnitsPerChunk = 0; // 0: not built
  DevBuf sDone, sIters, sStatus, sLastErr, sFinalErr, sHist, sClk, sDelta, sStepIter, sLambda, sTrust;
  DevBuf sFusedArgs; // the one-launch solve's descriptors, stashed per solve (mmx_fused.hip, kArgLazy)
  DevBuf sDiag; // [B][4] diagnostics of the last single-precision solve (mmx_problem_solve_diagnostics)
  DevBuf sDiagAcc; // [B][4] the wide route's accumulators behind it (mmx::StepParams::diagAcc)
  DevBuf sDiagErr0; // [B] ... and the first iteration's error (mmx::StepParams::diagErr0)
  bool diagValid = false;
  DevBuf sThetaAuto, sAutoMap, sAutoCount; // MMX_PRECISION_AUTO: initial parameters, the elements to escalate, their number
  mmx_tuning tuning{}; // mmx_problem_set_tuning
  int32_t lastRoute = MMX_ROUTE_AUTO;
  // The live-joint view (solveView below): the rig and the joint-indexed tables over the joints the solve can depend on,
  // renumbered.  Built by uploadProblemTables when it prunes something; what the one-launch, mixed, wave and tree kernels get.
  mmx::LiveJoints liveJoints;
  bool viewBuilt = false;
  mmx::RigDev vRig{};
  int32_t vNnz = 0;
  DevBuf vParent, vPreRot, vOffset, vPtOuter, vPtInner, vPtValue, vPtOffsets, vLevelOrder, vLevelStart, vPtEll, vJumpParent, vPtRowRec;
  DevBuf vUnitJoint, vUnitTin, vJointTin, vGenJoint, vGenTin, vEllipsoids, vLimits;
  DevBuf vSubSize, vDfsJoint, vLoadedPos, vPosUnitStart, vSrcs;
};

namespace {

// What the problem references, as the table builders of mmx_host_tables.hpp take it
mmx::ProblemTopology problemTopology(const mmx_problem* pb) {
  mmx::ProblemTopology p;
  p.Kp = pb->Kp;
  p.Ko = pb->Ko;
  p.posParent = pb->posParent;
  p.oriParent = pb->oriParent;
  p.instPos = pb->instPos;
  p.instOri = pb->instOri;
  p.unionPos = pb->unionPos;
  p.unionOri = pb->unionOri;
  p.blocks = pb->blocks;
  p.ellipsoids = pb->ellipsoids;
  p.limits = pb->limits;
  p.hasModel = pb->dev.hasModel != 0;
  return p;
}

// The host unit's loss record (mmx_constraint_intake.hpp) as the kernels take it
mmx::LossDev lossDev(const mmx::LossHost& l) {
  static_assert(
      sizeof(mmx::LossHost) == sizeof(mmx::LossDev) && offsetof(mmx::LossHost, type) == offsetof(mmx::LossDev, type) &&
          offsetof(mmx::LossHost, alpha) == offsetof(mmx::LossDev, alpha) && offsetof(mmx::LossHost, invC2) == offsetof(mmx::LossDev, invC2) &&
          offsetof(mmx::LossHost, c) == offsetof(mmx::LossDev, c),
      "loss layouts must match");
  mmx::LossDev d;
  std::memcpy(&d, &l, sizeof(d));
  return d;
}

// mmx_ellipsoid_limit + the joint words of JointTables (full or renumbered) = the device record
std::vector<mmx::EllipsoidDev> packEllipsoids(const std::vector<mmx_ellipsoid_limit>& ellipsoids, const mmx::JointTables& jt) {
  static_assert(sizeof(mmx_ellipsoid_limit) == 30 * 4 && sizeof(mmx::EllipsoidDev) == 32 * 4, "ellipsoid layouts");
  std::vector<mmx::EllipsoidDev> ed(ellipsoids.size());
  for (size_t i = 0; i < ed.size(); ++i) {
    std::memcpy(&ed[i], &ellipsoids[i], sizeof(mmx_ellipsoid_limit));
    ed[i].parent = jt.ellParent[i];
    ed[i].ellipsoidParent = jt.ellEllipsoidParent[i];
    ed[i].tinParent = jt.ellTinParent[i];
    ed[i].tinStop = jt.ellTinStop[i];
  }
  return ed;
}

// Uploads the live-joint view's tables (mmx::buildLiveView): what the solve kernels index by joint or by DFS position, over
// the joints the solve can depend on.  uploadProblemTables builds no view -- the kernels keep the full descriptors -- with
// per-instance constraint parents (their lists name full joint ids; the per-instance rig arrays are looked at per solve,
// solveView) and when nothing would be pruned.
int32_t uploadSolveView(mmx_problem* pb, const mmx::LiveView& lv) {
  static_assert(sizeof(mmx_parameter_limit) == sizeof(mmx::LimitDev), "limit layouts must match");
  pb->viewBuilt = false;
  const mmx::RigDerived& rd = lv.derived;
  MMX_HIP(upload(pb->vParent, lv.rig.parent));
  MMX_HIP(upload(pb->vPreRot, lv.rig.preRot));
  MMX_HIP(upload(pb->vOffset, lv.rig.offset));
  MMX_HIP(upload(pb->vPtOuter, lv.rig.ptOuter));
  MMX_HIP(upload(pb->vPtInner, lv.rig.ptInner));
  MMX_HIP(upload(pb->vPtValue, lv.rig.ptValue));
  MMX_HIP(upload(pb->vPtOffsets, lv.rig.ptOffsets));
  MMX_HIP(upload(pb->vLevelOrder, lv.order.levelOrder));
  MMX_HIP(upload(pb->vLevelStart, lv.order.levelStart));
  if (rd.ellOk) {
    MMX_HIP(upload(pb->vPtEll, rd.ell));
  }
  MMX_HIP(upload(pb->vJumpParent, rd.jumpParent));
  if (!rd.rowRec.empty()) {
    MMX_HIP(upload(pb->vPtRowRec, rd.rowRec));
  }
  MMX_HIP(upload(pb->vUnitJoint, lv.joints.unitJoint));
  MMX_HIP(upload(pb->vUnitTin, lv.joints.unitTin));
  MMX_HIP(upload(pb->vJointTin, lv.order.tin));
  MMX_HIP(upload(pb->vGenJoint, lv.joints.genJoint));
  MMX_HIP(upload(pb->vGenTin, lv.joints.genTin));
  MMX_HIP(upload(pb->vEllipsoids, packEllipsoids(pb->ellipsoids, lv.joints)));
  MMX_HIP(upload(pb->vLimits, lv.limits));
  MMX_HIP(upload(pb->vSubSize, lv.subSize));
  MMX_HIP(upload(pb->vDfsJoint, lv.dfsJoint));
  MMX_HIP(upload(pb->vLoadedPos, lv.loadedPos));
  MMX_HIP(upload(pb->vPosUnitStart, lv.posUnitStart));
  MMX_HIP(upload(pb->vSrcs, lv.slots));
  mmx::RigDev& v = pb->vRig;
  v = pb->rig->dev; // P, ptOffsetsNonZero (a dead row's offset moves nothing the solve reads), layoutJ = the full rig's count
  v.J = int32_t(lv.rig.parent.size());
  v.R = MMX_PARAMS_PER_JOINT * v.J;
  v.numLevels = int32_t(lv.order.levelStart.size()) - 1;
  v.parent = pb->vParent.as<int32_t>();
  v.preRot = pb->vPreRot.as<float>();
  v.offset = pb->vOffset.as<float>();
  v.ptOuter = pb->vPtOuter.as<int32_t>();
  v.ptInner = pb->vPtInner.as<int32_t>();
  v.ptValue = pb->vPtValue.as<float>();
  v.ptOffsets = pb->vPtOffsets.as<float>();
  v.levelOrder = pb->vLevelOrder.as<int32_t>();
  v.levelStart = pb->vLevelStart.as<int32_t>();
  v.ptEll = rd.ellOk ? pb->vPtEll.as<int4>() : nullptr;
  v.ptRowRec = rd.rowRec.empty() ? nullptr : pb->vPtRowRec.as<int4>();
  v.numRowRec = int32_t(rd.rowRec.size() / 4);
  v.jumpParent = pb->vJumpParent.as<int32_t>();
  v.jumpRounds = rd.jumpRounds;
  v.instPreRot = nullptr;
  v.instOffset = nullptr;
  pb->vNnz = lv.rig.ptOuter.back();
  pb->viewBuilt = true;
  return MMX_OK;
}

// Builds every table of the problem on the host (mmx_host_tables.hpp: pure index arithmetic, tested on the CPU), then
// uploads them and sets the descriptors.  A refusal comes out of the build, before anything on the device has changed.
int32_t uploadProblemTables(mmx_problem* pb) {
  const mmx_rig* rig = pb->rig;
  MMX_HIP(hipSetDevice(rig->device));
  // ---- build
  const mmx::HostTables& t = pb->tables;
  const mmx_rig_desc rd = rig->desc();
  const mmx::ProblemTopology topo = problemTopology(pb);
  std::string err;
  const mmx::JointTables jt = mmx::buildJointTables(topo, nullptr, t.tin, t.tout);
  const mmx::StructureLists sl = mmx::buildStructureLists(&rd, topo);
  mmx::FusedTables fused;
  int32_t rc = mmx::buildProblemFusedTables(&rd, t, topo, sl, fused, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  const mmx::ColumnProgram cp = mmx::buildColumnProgram(t, fused);
  const int32_t n = int32_t(fused.solveList.size());
  const int nbFused = mmx::fusedBlocksFor(n); // -1: beyond the fused instantiations (tables unused then)
  const mmx::SlotTables st = mmx::buildSlotTables(fused, nbFused > 0 ? nbFused : std::max((n + 15) / 16, 1));
  mmx::TermRuns runs;
  rc = mmx::buildTermRuns(fused, st, rig->J, runs, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  std::vector<uint32_t> terms, terms16;
  const size_t rounds = mmx::dealTermRuns(runs, 256, terms), rounds16 = mmx::dealTermRuns(runs, 1024, terms16);
  mmx::LimitTables lt = mmx::buildLimitTables(&rd, pb->limits, fused.solveList);
  mmx::ExplicitSolveLists xl = mmx::buildExplicitSolveLists(&rd, t, topo, sl.force);
  const int32_t G = int32_t(jt.genBlock.size()), NE = int32_t(pb->ellipsoids.size());
  const bool dense = mmx::tileStructureDense(fused, xl.list, G + NE);
  mmx::TileMasks tileMasks =
      mmx::eliminationTileMasks(std::min(n, 512), dense ? std::vector<uint8_t>() : mmx::buildRelatedness(&rd, fused, lt.limitPairs), dense);
  const std::vector<uint32_t> masks = mmx::packTileMasks(tileMasks);
  mmx::LiveJoints lj;
  const std::vector<int32_t> ref = mmx::referencedJoints(topo);
  mmx::buildLiveJoints(rig->parent.data(), rig->J, ref.data(), int32_t(ref.size()), lj);
  const bool wantView = !lj.identity() && !pb->instPos && !pb->instOri;
  const mmx::LiveView lv = wantView ? mmx::buildLiveView(&rd, t, fused, topo, lj, st.slots) : mmx::LiveView{};
  // ---- the host copies other entry points read
  pb->fused = std::move(fused);
  pb->limitPairs = std::move(lt.limitPairs);
  pb->solveN = int32_t(xl.list.size());
  pb->solveListV1 = std::move(xl.list);
  pb->solveListF64 = std::move(xl.sorted);
  pb->f64ListUnitsPerChunk = 0;
  pb->tileMasks = std::move(tileMasks);
  pb->liveJoints = std::move(lj);
  const mmx::FusedTables& f = pb->fused;
  // ---- upload
  static_assert(sizeof(mmx::ColumnSource) == sizeof(mmx::ColumnSourceDev), "ColumnSource layouts must match");
  static_assert(sizeof(mmx::JacRec) == sizeof(mmx::JacRecDev) && sizeof(mmx::JacRec) == 32, "JacRec layouts must match");
  MMX_HIP(upload(pb->dUnitJoint, jt.unitJoint));
  MMX_HIP(upload(pb->dUnitTin, jt.unitTin));
  MMX_HIP(upload(pb->dJointTin, t.tin));
  MMX_HIP(upload(pb->dGenJoint, jt.genJoint));
  MMX_HIP(upload(pb->dGenTin, jt.genTin));
  MMX_HIP(upload(pb->dGenBlock, jt.genBlock));
  MMX_HIP(upload(pb->dBlocks, pb->blockDev));
  MMX_HIP(upload(pb->dEllipsoids, packEllipsoids(pb->ellipsoids, jt)));
  MMX_HIP(upload(pb->dColStart, t.colStart));
  MMX_HIP(upload(pb->dColSources, t.colSources));
  MMX_HIP(upload(pb->dEnabledList, t.enabledList));
  MMX_HIP(upload(pb->dEnabledMask, t.enabled));
  MMX_HIP(upload(pb->dJacRecs, cp.recs));
  MMX_HIP(upload(pb->dMultiCols, cp.multi));
  MMX_HIP(upload(pb->dZeroCols, cp.zero));
  MMX_HIP(upload(pb->dSubSize, f.subSize));
  MMX_HIP(upload(pb->dDfsJoint, f.dfsJoint));
  MMX_HIP(upload(pb->dLoadedPos, st.loadedPos));
  MMX_HIP(upload(pb->dPosUnitStart, f.posUnitStart));
  MMX_HIP(upload(pb->dPosUnits, f.posUnits));
  MMX_HIP(upload(pb->dSolveList, f.solveList));
  MMX_HIP(upload(pb->dSrcStart, st.xStart));
  MMX_HIP(upload(pb->dSrcs, st.slots));
  MMX_HIP(upload(pb->dComb, runs.comb));
  MMX_HIP(upload(pb->dTerms, terms));
  MMX_HIP(upload(pb->dTerms16, terms16));
  MMX_HIP(upload(pb->dPairCols, lt.pairCols));
  MMX_HIP(upload(pb->dLimStart, lt.limStart));
  MMX_HIP(upload(pb->dLimOf, lt.limOf));
  MMX_HIP(upload(pb->dPairDest, lt.pairDest));
  MMX_HIP(upload(pb->dPairStart, lt.pairStart));
  MMX_HIP(upload(pb->dPairLim, lt.pairLim));
  MMX_HIP(upload(pb->dSolveListV1, pb->solveListV1));
  MMX_HIP(upload(pb->dSolveListF64, pb->solveListF64));
  MMX_HIP(upload(pb->dTileMasks, masks));
  MMX_HIP(upload(pb->dTileList, pb->tileMasks.tiles));
  // ---- descriptors
  mmx::ProblemDev& d = pb->dev;
  d.B = pb->B;
  d.Kp = pb->Kp;
  d.Ko = pb->Ko;
  d.U = pb->U;
  d.M = pb->M;
  d.n = int32_t(t.enabledList.size());
  d.unitJoint = pb->dUnitJoint.as<int32_t>();
  d.unitTin = pb->dUnitTin.as<int32_t>();
  d.jointTin = pb->dJointTin.as<int32_t>();
  d.numBlocks = int32_t(pb->blocks.size());
  d.G = G;
  d.blocks = pb->dBlocks.as<mmx::JointBlockDev>();
  d.genJoint = pb->dGenJoint.as<int32_t>();
  d.genTin = pb->dGenTin.as<int32_t>();
  d.genBlock = pb->dGenBlock.as<int32_t>();
  d.NE = NE;
  d.ellipsoids = pb->dEllipsoids.as<mmx::EllipsoidDev>();
  d.colStart = pb->dColStart.as<int32_t>();
  d.colSources = pb->dColSources.as<mmx::ColumnSourceDev>();
  d.enabledList = pb->dEnabledList.as<int32_t>();
  d.enabledMask = pb->dEnabledMask.as<uint8_t>();
  d.rowsJoint = 3 * pb->U + pb->genRows + 3 * NE;
  d.jacRecs = pb->dJacRecs.as<mmx::JacRecDev>();
  d.multiCols = pb->dMultiCols.as<int32_t>();
  d.zeroCols = pb->dZeroCols.as<int32_t>();
  d.numJacRecs = int32_t(cp.recs.size());
  d.numMultiCols = int32_t(cp.multi.size());
  d.numZeroCols = int32_t(cp.zero.size());
  mmx::FusedDev& fd = pb->fdev;
  fd.U = pb->U;
  fd.Kp = pb->Kp;
  fd.n = n;
  fd.nsrc = int32_t(st.slots.size());
  fd.slotBase = st.slotBase;
  fd.nnz = rig->ptOuter.back();
  fd.subSize = pb->dSubSize.as<int32_t>();
  fd.dfsJoint = pb->dDfsJoint.as<int32_t>();
  fd.loadedPos = pb->dLoadedPos.as<int32_t>();
  fd.numLoaded = int32_t(st.loadedPos.size());
  fd.unitJoint = pb->dUnitJoint.as<int32_t>();
  fd.posUnitStart = pb->dPosUnitStart.as<int32_t>();
  fd.posUnits = pb->dPosUnits.as<int32_t>();
  fd.solveList = pb->dSolveList.as<int32_t>();
  fd.srcStart = pb->dSrcStart.as<int32_t>();
  fd.srcs = pb->dSrcs.as<mmx::ColumnSourceDev>();
  fd.comb = pb->dComb.as<int32_t>();
  fd.numComb = int32_t(runs.comb.size() / 3);
  fd.numCells = runs.numCells;
  fd.gTerms = pb->dTerms.as<uint4>();
  fd.termRounds = int32_t(rounds);
  fd.gTerms16 = pb->dTerms16.as<uint4>();
  fd.termRounds16 = int32_t(rounds16);
  fd.pairCols = pb->dPairCols.as<int32_t>();
  fd.numLimits = int32_t(pb->limits.size());
  fd.limStart = pb->dLimStart.as<int32_t>();
  fd.limOf = pb->dLimOf.as<int32_t>();
  fd.numPairDests = int32_t(lt.pairDest.size());
  fd.pairDest = pb->dPairDest.as<int32_t>();
  fd.pairStart = pb->dPairStart.as<int32_t>();
  fd.pairLim = pb->dPairLim.as<int32_t>();
  fd.GT = G + NE;
  fd.genRows = fd.GT > 0 ? d.rowsJoint - 3 * pb->U : 0;
  fd.tileList = pb->dTileList.as<int32_t>();
  fd.numTiles = int32_t(pb->tileMasks.tiles.size());
  pb->viewBuilt = false;
  return wantView ? uploadSolveView(pb, lv) : MMX_OK;
}

// What the one-launch solve, its mixed-precision instantiation, the wave route and the tree kernels are launched with: the
// live-joint view of the problem (uploadSolveView) -- rig, problem and table descriptors TOGETHER, so that a table and a rig
// can never disagree -- or the full descriptors when nothing is pruned: no view built, switched off (mmx_tuning::
// joint_pruning), or per-instance rigs / constraint parents set (their arrays are indexed by full joint id).
// Every host decision (routes, instantiations, LDS budgets) keeps reading the full rig's joint count.
struct SolveView {
  mmx::RigDev rig;
  mmx::ProblemDev pb;
  mmx::FusedDev fd;
};
bool solveViewActive(const mmx_problem* pb) {
  return pb->viewBuilt && pb->tuning.joint_pruning == 0 && pb->rigDev.instPreRot == nullptr && pb->rigDev.instOffset == nullptr &&
      pb->dev.instPosParent == nullptr && pb->dev.instOriParent == nullptr;
}
SolveView solveView(const mmx_problem* pb) {
  SolveView v{pb->rigDev, pb->dev, pb->fdev};
  if (!solveViewActive(pb)) {
    return v;
  }
  v.rig = pb->vRig;
  v.pb.unitJoint = pb->vUnitJoint.as<int32_t>();
  v.pb.unitTin = pb->vUnitTin.as<int32_t>();
  v.pb.jointTin = pb->vJointTin.as<int32_t>();
  v.pb.genJoint = pb->vGenJoint.as<int32_t>();
  v.pb.genTin = pb->vGenTin.as<int32_t>();
  v.pb.ellipsoids = pb->vEllipsoids.as<mmx::EllipsoidDev>();
  v.pb.limits = pb->vLimits.as<mmx::LimitDev>();
  v.fd.nnz = pb->vNnz;
  v.fd.subSize = pb->vSubSize.as<int32_t>();
  v.fd.dfsJoint = pb->vDfsJoint.as<int32_t>();
  v.fd.loadedPos = pb->vLoadedPos.as<int32_t>();
  v.fd.unitJoint = pb->vUnitJoint.as<int32_t>();
  v.fd.posUnitStart = pb->vPosUnitStart.as<int32_t>();
  v.fd.srcs = pb->vSrcs.as<mmx::ColumnSourceDev>();
  return v;
}

bool fusedUsable(const mmx_problem* pb) {
  const int nb = mmx::fusedBlocksFor(pb->fdev.n);
  if (nb < 0) {
    return false;
  }
  // (the further joint-constraint blocks and ellipsoid limits ride along as a dense block of rows in LDS -- fdev.GT /
  // genRows -- while they fit; MMX_ROUTE_EXPLICIT_JACOBIAN sends them to the explicit-Jacobian kernels)
  return pb->rig->J < 4096 &&
      mmx::fusedLdsBytes(nb, pb->rig->J, pb->rig->P, pb->U, pb->fdev.nsrc, pb->fdev.n, pb->fdev.numCells, true, pb->fdev.GT, pb->fdev.genRows, true, mmx::fusedCsrFloats(pb->rig->J, pb->fdev.nnz)) +
          size_t(8) * size_t(pb->rig->J + pb->rig->P) <=
      160 * 1024;
}

// H and g of the explicit-Jacobian solver from the tree moments instead of the dense J (treeNormalEquationsKernel):
// the same solve list on both sides, everything within the kernels' LDS
bool treeNormalEquationsUsable(const mmx_problem* pb) {
  // (limit / model-parameter rows ride along: evaluated on the fly from theta like in the fused solve; the further joint
  // error functions and ellipsoid limits as a dense block of rows in LDS while it fits)
  return pb->U > 0 && pb->fdev.n > 0 && pb->fdev.n <= 512 && pb->fdev.nsrc < 4096 &&
      pb->fused.solveList == pb->solveListV1 &&
      mmx::treeNormalEquationsLdsBytes(pb->rig->J, pb->rig->P, pb->U, pb->fdev.nsrc, pb->fdev.n, pb->fdev.GT, pb->fdev.genRows) <= 160 * 1024 - 64 &&
      mmx::treeRefineLdsBytes(pb->rig->J, pb->rig->P, pb->U, pb->fdev.n, pb->fdev.genRows) <= 160 * 1024 - 64;
}

// profiling aid (one of the library's two environment reads; the other is MMX_NO_ROCTX, the marker switch): per-phase cycle
// counters of workgroup 0, printed to stderr after the solve.  Not on any product path: the clocked instantiation is a
// separate kernel.
// refinement steps a solve may take per iteration (mmx_tuning::max_refinement_steps: 0 = the default, three; -1 = none)
int32_t refineSteps(const mmx_problem* pb) {
  const int32_t m = pb->tuning.max_refinement_steps;
  return m == 0 ? 3 : (m < 0 ? 0 : (m > 3 ? 3 : m));
}

bool phaseClocksWanted() {
  static const bool wanted = getenv("MMX_PHASE_CLOCKS") != nullptr;
  return wanted;
}

// MMX_PHASE_STOP=<stamp> beside MMX_PHASE_CLOCKS: the clocked instantiation's workgroups end at that stamp of their first
// iteration (slot 31 of the clock array carries stamp + 1) -- the solve's outputs are then meaningless; for counter passes only
hipError_t armPhaseStop(long long* clk, hipStream_t s) {
  static const long long stop = getenv("MMX_PHASE_STOP") != nullptr ? atoll(getenv("MMX_PHASE_STOP")) + 1 : 0;
  return stop > 0 ? hipMemcpyAsync(clk + 31, &stop, sizeof(long long), hipMemcpyHostToDevice, s) : hipSuccess;
}

int32_t checkProblem(const mmx_problem* pb, bool needConstraints) {
  // hipGetLastError() is per thread and shared with every other user of the runtime in this
  // process (torch probes devices / pointers and leaves benign errors behind): start clean so that
  // the launchers below only ever report their own failures
  (void)hipGetLastError();
  if (pb == nullptr || pb->rig == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "problem handle is null");
  }
  if (needConstraints && !pb->haveConstraints && pb->U > 0) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_problem_set_constraints has not been called");
  }
  return MMX_OK;
}

} // namespace

extern "C" {

void mmx_gn_options_default(mmx_gn_options* o) {
  if (o == nullptr) {
    return;
  }
  o->min_iterations = 1; // SolverOptions (momentum/solver/solver.h:19-34)
  o->max_iterations = 2;
  o->threshold = 1.0f;
  o->regularization = 0.05f; // GaussNewtonSolverBaseOptions (gauss_newton_solver.h:17-33)
  o->do_line_search = 0;
  o->step_rule = MMX_STEP_GN_FIXED_LAMBDA;
  o->lm_lambda_min = 1e-6f;
  o->lm_lambda_max = 1e6f;
  o->lm_up = 4.0f;
  o->lm_down = 0.5f;
  o->trust_region_radius = 1.0f; // TrustRegionQROptions::trustRegionRadius_ (trust_region_qr.h:24)
  o->precision = MMX_PRECISION_F32;
  o->precision_bound = 1e-5f;
}

int32_t mmx_abi_version(void) {
  return MMX_ABI_VERSION;
}

const char* mmx_last_error(void) {
  return g_lastError.c_str();
}

int32_t mmx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int32_t mmx_host_tables(
    const mmx_rig_desc* desc,
    const uint8_t* enabled,
    int32_t* level,
    int32_t* tin,
    int32_t* tout,
    uint8_t* active_joint_params,
    int32_t* enabled_list,
    int32_t* num_enabled) {
  mmx::HostTables t;
  std::string err;
  const int32_t rc = mmx::buildHostTables(desc, enabled, t, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  if (level) {
    std::memcpy(level, t.level.data(), sizeof(int32_t) * t.J);
  }
  if (tin) {
    std::memcpy(tin, t.tin.data(), sizeof(int32_t) * t.J);
  }
  if (tout) {
    std::memcpy(tout, t.tout.data(), sizeof(int32_t) * t.J);
  }
  if (active_joint_params) {
    std::memcpy(active_joint_params, t.activeJointParams.data(), t.activeJointParams.size());
  }
  if (enabled_list) {
    std::memcpy(enabled_list, t.enabledList.data(), sizeof(int32_t) * t.enabledList.size());
  }
  if (num_enabled) {
    *num_enabled = int32_t(t.enabledList.size());
  }
  return MMX_OK;
}

int32_t mmx_host_elimination_order(const mmx_rig_desc* desc, const uint8_t* enabled, int32_t* order, int32_t* num_enabled) {
  mmx::HostTables t;
  std::string err;
  const int32_t rc = mmx::buildHostTables(desc, enabled, t, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  if (order) {
    std::memcpy(order, t.eliminationList.data(), sizeof(int32_t) * t.eliminationList.size());
  }
  if (num_enabled) {
    *num_enabled = int32_t(t.eliminationList.size());
  }
  return MMX_OK;
}

int32_t mmx_host_live_joints(const mmx_rig_desc* desc, int32_t n, const int32_t* joints, uint8_t* live, int32_t* compact_of, int32_t* num_live) {
  std::string err;
  const int32_t rc = mmx::validateRigDesc(desc, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  if (n < 0 || (n > 0 && joints == nullptr)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_host_live_joints: negative count or null joint list");
  }
  for (int32_t i = 0; i < n; ++i) {
    if (joints[i] < 0 || joints[i] >= desc->num_joints) {
      return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_host_live_joints: joint index out of range");
    }
  }
  mmx::LiveJoints lj;
  mmx::buildLiveJoints(desc->parent, desc->num_joints, joints, n, lj);
  if (live) {
    std::memcpy(live, lj.live.data(), lj.live.size());
  }
  if (compact_of) {
    std::memcpy(compact_of, lj.compactOf.data(), sizeof(int32_t) * lj.compactOf.size());
  }
  if (num_live) {
    *num_live = lj.numLive;
  }
  return MMX_OK;
}

int32_t mmx_host_tile_structure(int32_t n, const uint8_t* related, uint32_t* row_mask, uint32_t* col_mask, int64_t* products) {
  if (n < 0 || n > 512 || (n > 0 && related == nullptr)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_host_tile_structure: n outside 0..512 or related is null");
  }
  const std::vector<uint8_t> rel(related, related + size_t(n) * size_t(n));
  const mmx::TileMasks m = mmx::eliminationTileMasks(n, rel, false);
  for (int i = 0; i < 32; ++i) {
    if (row_mask) {
      row_mask[i] = m.rowMask[i];
    }
    if (col_mask) {
      col_mask[i] = m.colMask[i];
    }
  }
  if (products) {
    *products = m.products;
  }
  return MMX_OK;
}

int32_t mmx_host_tile_level_schedule(int32_t n, const uint8_t* related, int32_t* steps) {
  if (n < 0 || n > 512 || (n > 0 && related == nullptr) || steps == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_host_tile_level_schedule: n outside 0..512, or related / steps is null");
  }
  const std::vector<uint8_t> rel(related, related + size_t(n) * size_t(n));
  const mmx::TileMasks m = mmx::eliminationTileMasks(n, rel, false);
  if (m.levelSteps.size() > size_t(1 + 4 * 32)) {
    return fail(MMX_ERR_UNSUPPORTED, "mmx_host_tile_level_schedule: more than 32 steps");
  }
  std::copy(m.levelSteps.begin(), m.levelSteps.end(), steps);
  return MMX_OK;
}

int32_t mmx_host_f64_assembly_list(
    const mmx_rig_desc* desc,
    const int32_t* solve_list,
    int32_t n,
    const int32_t* pos_parent,
    int32_t num_pos,
    const int32_t* ori_parent,
    int32_t num_ori,
    int32_t units_per_chunk,
    uint32_t* groups,
    int32_t* num_groups,
    int32_t* extra,
    int32_t* num_extra,
    int32_t* chunk_start,
    int32_t* num_chunks) {
  if (n < 0 || num_pos < 0 || num_ori < 0 || units_per_chunk <= 0 || units_per_chunk > 64 || (n > 0 && solve_list == nullptr) ||
      (num_pos > 0 && pos_parent == nullptr) || (num_ori > 0 && ori_parent == nullptr)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_host_f64_assembly_list: sizes / pointers");
  }
  mmx::HostTables t;
  std::string err;
  const int32_t rc = mmx::buildHostTables(desc, nullptr, t, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  for (int32_t i = 0; i < n; ++i) {
    if (solve_list[i] < 0 || solve_list[i] >= t.P) {
      return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_host_f64_assembly_list: parameter index out of range");
    }
  }
  for (int32_t i = 0; i < num_pos + num_ori; ++i) {
    const int32_t j = i < num_pos ? pos_parent[i] : ori_parent[i - num_pos];
    if (j < 0 || j >= t.J) {
      return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_host_f64_assembly_list: joint index out of range");
    }
  }
  mmx::F64AssemblyListHost h;
  if (!mmx::buildF64AssemblyListHost(t, std::vector<int32_t>(solve_list, solve_list + n), pos_parent, num_pos, ori_parent, num_ori, units_per_chunk, h)) {
    return fail(MMX_ERR_UNSUPPORTED, "mmx_host_f64_assembly_list: more than 8191 sources of one column apply to one constraint");
  }
  const int32_t chunks = (num_pos + 3 * num_ori + units_per_chunk - 1) / units_per_chunk;
  // sizes first (null arrays: a query), then the arrays when the caller's capacities (passed in the counters) suffice
  const int32_t capG = num_groups ? *num_groups : 0, capE = num_extra ? *num_extra : 0;
  if (num_groups) {
    *num_groups = int32_t(h.groups.size() / 2);
  }
  if (num_extra) {
    *num_extra = int32_t(h.extra.size());
  }
  if (num_chunks) {
    *num_chunks = chunks;
  }
  if (groups != nullptr && capG >= int32_t(h.groups.size() / 2)) {
    std::copy(h.groups.begin(), h.groups.end(), groups);
  }
  if (extra != nullptr && capE >= int32_t(h.extra.size())) {
    std::copy(h.extra.begin(), h.extra.end(), extra);
  }
  if (chunk_start != nullptr) {
    std::copy(h.chunkStart.begin(), h.chunkStart.end(), chunk_start); // [2 chunks + 1]
  }
  return MMX_OK;
}

int32_t mmx_problem_tile_structure(mmx_problem* pb, uint32_t* row_mask, uint32_t* col_mask, int32_t* num_blocks, int32_t* num_tiles, int64_t* products) {
  if (pb == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "problem is null");
  }
  const mmx::TileMasks& m = pb->tileMasks;
  for (int i = 0; i < 32; ++i) {
    if (row_mask) {
      row_mask[i] = m.rowMask[i];
    }
    if (col_mask) {
      col_mask[i] = m.colMask[i];
    }
  }
  if (num_blocks) {
    *num_blocks = m.NB;
  }
  if (num_tiles) {
    *num_tiles = int32_t(m.tiles.size());
  }
  if (products) {
    *products = m.products;
  }
  return MMX_OK;
}

int32_t mmx_rig_create(const mmx_rig_desc* d, int32_t device, mmx_rig** out) {
  MMX_ZONE("mmx_rig_create");
  if (out == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "out is null");
  }
  *out = nullptr;
  mmx::HostTables topo;
  std::string err;
  int32_t rc = mmx::buildHostTables(d, nullptr, topo, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  const int ndev = mmx_device_count();
  if (ndev <= 0) {
    return fail(MMX_ERR_NO_DEVICE, "no HIP device visible; the MI355X path has no CPU fallback");
  }
  if (device < 0 || device >= ndev) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "device index out of range");
  }
  mmx_rig* r = new (std::nothrow) mmx_rig();
  if (r == nullptr) {
    return fail(MMX_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  r->device = device;
  r->J = d->num_joints;
  r->P = d->num_params;
  const int32_t R = MMX_PARAMS_PER_JOINT * r->J;
  r->parent.assign(d->parent, d->parent + r->J);
  r->preRot.assign(d->pre_rotation, d->pre_rotation + 4 * r->J);
  r->offset.assign(d->translation_offset, d->translation_offset + 3 * r->J);
  r->ptOuter.assign(d->pt_outer, d->pt_outer + R + 1);
  const int32_t nnz = r->ptOuter[R];
  r->ptInner.assign(d->pt_inner, d->pt_inner + nnz);
  r->ptValue.assign(d->pt_value, d->pt_value + nnz);
  if (d->pt_offsets != nullptr) {
    r->ptOffsets.assign(d->pt_offsets, d->pt_offsets + R);
  } else {
    r->ptOffsets.assign(R, 0.f);
  }
  r->topo = std::move(topo);
  auto cleanup = [&](int32_t code) {
    delete r;
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) {
    return cleanup(fail(MMX_ERR_DEVICE, "hipSetDevice failed"));
  }
#define UP(buf, vec)                                                             \
  do {                                                                           \
    hipError_t e_ = upload(buf, vec);                                            \
    if (e_ != hipSuccess) {                                                      \
      return cleanup(fail(MMX_ERR_DEVICE, std::string("rig upload: ") + hipGetErrorString(e_))); \
    }                                                                            \
  } while (0)
  UP(r->dParent, r->parent);
  UP(r->dPreRot, r->preRot);
  UP(r->dOffset, r->offset);
  UP(r->dPtOuter, r->ptOuter);
  UP(r->dPtInner, r->ptInner);
  UP(r->dPtValue, r->ptValue);
  UP(r->dPtOffsets, r->ptOffsets);
  UP(r->dLevelOrder, r->topo.levelOrder);
  UP(r->dLevelStart, r->topo.levelStart);
  // two-slot ELL copy of the parameter transform, the packed level/parent table of the J-assembly kernel and the records of
  // the non-empty transform rows (deriveRigTables)
  const mmx::RigDerived rd = mmx::deriveRigTables(r->J, r->P, r->parent, r->ptOuter, r->ptInner, r->ptValue, int32_t(r->topo.levelStart.size()) - 1);
  const bool ellOk = rd.ellOk;
  const std::vector<int32_t>& rowRec = rd.rowRec;
  if (ellOk) {
    UP(r->dPtEll, rd.ell);
  }
  UP(r->dJumpParent, rd.jumpParent);
  if (!rowRec.empty()) {
    UP(r->dPtRowRec, rowRec);
  }
#undef UP
  mmx::RigDev& dv = r->dev;
  dv.ptRowRec = rowRec.empty() ? nullptr : r->dPtRowRec.as<int4>();
  dv.numRowRec = int32_t(rowRec.size() / 4);
  dv.ptEll = ellOk ? r->dPtEll.as<int4>() : nullptr;
  dv.jumpParent = r->dJumpParent.as<int32_t>();
  dv.jumpRounds = rd.jumpRounds;
  dv.J = r->J;
  dv.layoutJ = r->J;
  dv.P = r->P;
  dv.R = R;
  dv.numLevels = int32_t(r->topo.levelStart.size()) - 1;
  dv.parent = r->dParent.as<int32_t>();
  dv.preRot = r->dPreRot.as<float>();
  dv.offset = r->dOffset.as<float>();
  dv.ptOuter = r->dPtOuter.as<int32_t>();
  dv.ptInner = r->dPtInner.as<int32_t>();
  dv.ptValue = r->dPtValue.as<float>();
  dv.ptOffsets = r->dPtOffsets.as<float>();
  dv.ptOffsetsNonZero = 0;
  for (float v : r->ptOffsets) {
    dv.ptOffsetsNonZero |= v != 0.f ? 1 : 0;
  }
  dv.levelOrder = r->dLevelOrder.as<int32_t>();
  dv.levelStart = r->dLevelStart.as<int32_t>();
  *out = r;
  return MMX_OK;
}

void mmx_rig_destroy(mmx_rig* rig) {
  if (rig != nullptr) {
    (void)hipSetDevice(rig->device);
    delete rig;
  }
}

int32_t mmx_rig_num_joints(const mmx_rig* rig) {
  return rig ? rig->J : 0;
}
int32_t mmx_rig_num_params(const mmx_rig* rig) {
  return rig ? rig->P : 0;
}

int32_t mmx_problem_create(
    mmx_rig* rig,
    int32_t batch,
    int32_t num_pos,
    const int32_t* pos_parent,
    int32_t num_ori,
    const int32_t* ori_parent,
    mmx_problem** out) {
  MMX_ZONE("mmx_problem_create");
  if (out == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "out is null");
  }
  *out = nullptr;
  if (rig == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "rig handle is null");
  }
  if (batch <= 0 || num_pos < 0 || num_ori < 0) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "batch must be > 0 and constraint counts >= 0");
  }
  if ((num_pos > 0 && pos_parent == nullptr) || (num_ori > 0 && ori_parent == nullptr)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "constraint parent array is null");
  }
  if (!mmx::jointsInRange(pos_parent, size_t(num_pos), rig->J)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "position constraint parent joint out of range");
  }
  if (!mmx::jointsInRange(ori_parent, size_t(num_ori), rig->J)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "orientation constraint parent joint out of range");
  }
  mmx_problem* pb = new (std::nothrow) mmx_problem();
  if (pb == nullptr) {
    return fail(MMX_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  pb->rig = rig;
  pb->B = batch;
  pb->Kp = num_pos;
  pb->Ko = num_ori;
  pb->U = num_pos + 3 * num_ori;
  pb->M = 3 * pb->U;
  pb->dev.lossPos = mmx::LossDev{0, 2.f, 1.f, 1.f};
  pb->dev.lossOri = mmx::LossDev{0, 2.f, 1.f, 1.f};
  if (num_pos > 0) {
    pb->posParent.assign(pos_parent, pos_parent + num_pos);
  }
  if (num_ori > 0) {
    pb->oriParent.assign(ori_parent, ori_parent + num_ori);
  }
  pb->tables = rig->topo; // all parameters enabled
  pb->rigDev = rig->dev;
  pb->dev.wPos = 1.f;
  pb->dev.wOri = 1.f;
  const int32_t rc = uploadProblemTables(pb);
  if (rc != MMX_OK) {
    delete pb;
    return rc;
  }
  *out = pb;
  return MMX_OK;
}

void mmx_problem_destroy(mmx_problem* pb) {
  if (pb != nullptr) {
    if (pb->rig != nullptr) {
      (void)hipSetDevice(pb->rig->device);
    }
    delete pb;
  }
}

int32_t mmx_problem_num_rows(const mmx_problem* pb) {
  return pb ? pb->M : 0;
}
int32_t mmx_problem_batch(const mmx_problem* pb) {
  return pb ? pb->B : 0;
}

int32_t mmx_problem_set_tuning(mmx_problem* pb, const mmx_tuning* tuning) {
  int32_t rc = checkProblem(pb, false);
  if (rc != MMX_OK) {
    return rc;
  }
  if (tuning == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "tuning is null");
  }
  if (tuning->route < MMX_ROUTE_AUTO || tuning->route > MMX_ROUTE_WAVE) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_tuning::route: unknown MMX_ROUTE_* value");
  }
  if (tuning->max_refinement_steps < -1 || tuning->max_refinement_steps > 3) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_tuning::max_refinement_steps: -1 (none), 0 (default) or 1..3");
  }
  if (!(tuning->mixed_tolerance >= 0.f) || tuning->mixed_tolerance > 1e-2f || tuning->mixed_max_cg < 0 || tuning->mixed_max_cg > 64) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_tuning::mixed_tolerance: 0 (default) or (0, 1e-2]; mixed_max_cg: 0 (default) or 1..64");
  }
  if (tuning->joint_pruning != 0 && tuning->joint_pruning != -1) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_tuning::joint_pruning: 0 (on) or -1 (off)");
  }
  for (int32_t r : tuning->reserved) {
    if (r != 0) {
      return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_tuning::reserved must be zero");
    }
  }
  pb->tuning = *tuning;
  return MMX_OK;
}

int32_t mmx_problem_last_route(const mmx_problem* pb) {
  return pb != nullptr ? pb->lastRoute : MMX_ROUTE_AUTO;
}

int32_t mmx_problem_num_solve_joints(const mmx_problem* pb) {
  if (pb == nullptr || pb->rig == nullptr) {
    return 0;
  }
  return solveViewActive(pb) ? pb->liveJoints.numLive : pb->rig->J;
}

int32_t mmx_problem_set_enabled(mmx_problem* pb, const uint8_t* enabled) {
  MMX_ZONE("mmx_problem_set_enabled");
  int32_t rc = checkProblem(pb, false);
  if (rc != MMX_OK) {
    return rc;
  }
  if (enabled == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "enabled is null");
  }
  // an unchanged mask leaves every table as it is (callers like Solver.solve set it before every solve; the rebuild
  // is host bookkeeping plus some thirty synchronous uploads)
  if (!pb->tablesDirty && pb->tables.enabled.size() == size_t(pb->rig->P)) {
    bool same = true;
    for (size_t p = 0; p < pb->tables.enabled.size() && same; ++p) {
      same = (pb->tables.enabled[p] != 0) == (enabled[p] != 0);
    }
    if (same) {
      return MMX_OK;
    }
  }
  const mmx_rig_desc d = pb->rig->desc();
  std::string err;
  mmx::HostTables t;
  rc = mmx::buildHostTables(&d, enabled, t, err);
  if (rc != MMX_OK) {
    return fail(rc, err);
  }
  pb->tables = std::move(t);
  return uploadProblemTables(pb);
}

int32_t mmx_problem_set_instance_rig(mmx_problem* pb, const float* translation_offset, const float* pre_rotation, int32_t memory, void* stream) {
  MMX_ZONE("mmx_problem_set_instance_rig");
  int32_t rc = checkProblem(pb, false);
  if (rc != MMX_OK) {
    return rc;
  }
  if (memory != MMX_MEM_HOST && memory != MMX_MEM_DEVICE) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "instance rig: unknown memory space");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  const size_t B = size_t(pb->B), J = size_t(pb->rig->J);
  Staging stage(memory, static_cast<hipStream_t>(stream));
  const float *off = nullptr, *pre = nullptr;
  MMX_HIP(stage.bring(pb->oInstOffset, translation_offset, B * J * 3, off));
  MMX_HIP(stage.bring(pb->oInstPreRot, pre_rotation, B * J * 4, pre));
  MMX_HIP(stage.finish());
  pb->rigDev.instOffset = off;
  pb->rigDev.instPreRot = pre;
  return MMX_OK;
}

int32_t mmx_problem_set_instance_parents(mmx_problem* pb, const int32_t* pos_parent, const int32_t* ori_parent, int32_t memory, void* stream) {
  MMX_ZONE("mmx_problem_set_instance_parents");
  int32_t rc = checkProblem(pb, false);
  if (rc != MMX_OK) {
    return rc;
  }
  if (memory != MMX_MEM_HOST && memory != MMX_MEM_DEVICE) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "instance parents: unknown memory space");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t B = size_t(pb->B);
  // host view of the lists (device input is read back: the integer bookkeeping is host work)
  std::vector<int32_t> hp, ho;
  auto fetch = [&](const int32_t* src, size_t count, std::vector<int32_t>& dst) -> hipError_t {
    dst.clear();
    if (src == nullptr || count == 0) {
      return hipSuccess;
    }
    dst.resize(count);
    if (memory == MMX_MEM_HOST) {
      std::memcpy(dst.data(), src, count * sizeof(int32_t));
      return hipSuccess;
    }
    hipError_t e = hipMemcpyAsync(dst.data(), src, count * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
  };
  MMX_HIP(fetch(pos_parent, B * size_t(pb->Kp), hp));
  MMX_HIP(fetch(ori_parent, B * size_t(pb->Ko), ho));
  // everything is validated before anything is modified
  mmx::InstanceParentsIntake in = mmx::intakeInstanceParents(
      pb->rig->J, hp, ho, memory == MMX_MEM_HOST,
      {pb->instPos, pb->instOri, pb->unionPos, pb->unionOri, pb->instParentsFromHost, pb->instPosHost, pb->instOriHost, pb->tablesDirty});
  if (in.code != MMX_OK) {
    return fail(in.code, in.message);
  }
  if (in.unchanged) {
    return MMX_OK;
  }
  Staging stage(memory, s);
  const int32_t *dp = nullptr, *dq = nullptr;
  MMX_HIP(stage.bring(pb->oInstPosParent, pos_parent, hp.size(), dp));
  MMX_HIP(stage.bring(pb->oInstOriParent, ori_parent, ho.size(), dq));
  MMX_HIP(stage.finish());
  pb->dev.instPosParent = dp;
  pb->dev.instOriParent = dq;
  pb->instPos = dp != nullptr;
  pb->instOri = dq != nullptr;
  pb->instParentsFromHost = memory == MMX_MEM_HOST;
  pb->instPosHost = std::move(hp);
  pb->instOriHost = std::move(ho);
  if (in.sameTables) {
    return MMX_OK;
  }
  pb->tablesDirty = true;
  pb->unionPos = std::move(in.unionPos);
  pb->unionOri = std::move(in.unionOri);
  rc = uploadProblemTables(pb); // solve list, structurally zero columns: over the union of the batch
  if (rc != MMX_OK) {
    return rc;
  }
  pb->tablesDirty = false;
  return MMX_OK;
}

int32_t mmx_problem_set_constraints_sized(mmx_problem* pb, const mmx_constraint_data* c, size_t dataSize, void* stream) {
  if (c == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "constraint data is null");
  }
  // the layout every ABI since 1 shares ends with the `memory` field
  if (dataSize < offsetof(mmx_constraint_data, memory) + sizeof(int32_t)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_problem_set_constraints_sized: data_size is smaller than any mmx_constraint_data");
  }
  if (dataSize > sizeof(mmx_constraint_data)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_problem_set_constraints_sized: data_size is larger than this library's mmx_constraint_data (caller built against a newer ABI)");
  }
  mmx_constraint_data full;
  std::memset(&full, 0, sizeof(full)); // fields the caller's header did not have: absent
  std::memcpy(&full, c, dataSize);
  return mmx_problem_set_constraints(pb, &full, stream);
}

int32_t mmx_problem_set_constraints(mmx_problem* pb, const mmx_constraint_data* c, void* stream) {
  MMX_ZONE("mmx_problem_set_constraints");
  MMX_TRY(checkProblem(pb, false));
  // ---- every check, every derived integer and the comparison with the last accepted call (mmx_constraint_intake.cpp):
  // everything is validated before anything is modified
  const mmx_rig_desc rigDesc = pb->rig->desc();
  mmx::ConstraintIntake in =
      mmx::intakeConstraints(rigDesc, pb->Kp, pb->Ko, c, {pb->blocks, pb->ellipsoids, pb->limits, pb->dev.hasModel != 0, pb->tablesDirty});
  if (in.code != MMX_OK) {
    return fail(in.code, in.message);
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  mmx::ProblemDev& d = pb->dev;
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P);
  // ---- the payload.  From here on the problem is modified; should a device call fail half-way, tablesDirty -- set before the
  // handle's topology first differs from the derived tables -- keeps them from being trusted by the next call.
  Staging stage(c->memory, static_cast<hipStream_t>(stream));
  MMX_HIP(stage.bring(pb->oPosOffset, c->pos_offset, B * pb->Kp * 3, d.posOffset));
  MMX_HIP(stage.bring(pb->oPosTarget, c->pos_target, B * pb->Kp * 3, d.posTarget));
  MMX_HIP(stage.bring(pb->oPosWeight, c->pos_weight, B * pb->Kp, d.posWeight));
  MMX_HIP(stage.bring(pb->oOriOffset, c->ori_offset, B * pb->Ko * 4, d.oriOffset));
  MMX_HIP(stage.bring(pb->oOriTarget, c->ori_target, B * pb->Ko * 4, d.oriTarget));
  MMX_HIP(stage.bring(pb->oOriWeight, c->ori_weight, B * pb->Ko, d.oriWeight));
  // per-element error-function weights (errorFunctionWeights[iBatch][...] of the batched driver)
  MMX_HIP(stage.bring(pb->oFnWeights, c->function_weights, B * size_t(in.fnCols), d.fnWeights));
  MMX_HIP(stage.bring(pb->oMpTarget, c->model_target, B * P, d.mpTarget));
  MMX_HIP(stage.bring(pb->oMpWeights, c->model_weights, B * P, d.mpWeights));
  if (in.blocksChanged) {
    pb->tablesDirty = true;
    pb->blocks = std::move(in.blocks);
    pb->blockPayload.clear();
    for (size_t i = 0; i < pb->blocks.size(); ++i) {
      pb->blockPayload.push_back(std::make_unique<mmx_problem::BlockPayload>());
    }
  }
  pb->blockDev.assign(pb->blocks.size(), mmx::JointBlockDev{});
  for (size_t i = 0; i < pb->blocks.size(); ++i) {
    const mmx_joint_constraint_block& jb = c->joint_blocks[i];
    mmx_problem::BlockPayload& h = *pb->blockPayload[i];
    mmx::JointBlockDev& k = pb->blockDev[i];
    k.type = jb.type;
    k.count = jb.count;
    k.first = in.blockRows[i].first;
    k.rowStart = in.blockRows[i].rowStart;
    k.fw = jb.function_weight;
    k.loss = lossDev(in.blockRows[i].loss);
    k.nearClip = in.blockRows[i].nearClip;
    const size_t cnt = B * size_t(jb.count);
    MMX_HIP(stage.bring(h.oLocalPoint, jb.local_point, 3 * cnt, k.localPoint));
    MMX_HIP(stage.bring(h.oLocalDir, jb.local_dir, 3 * cnt, k.localDir));
    MMX_HIP(stage.bring(h.oGlobal, jb.global, 3 * cnt, k.global));
    MMX_HIP(stage.bring(h.oPlaneD, jb.plane_d, cnt, k.planeD));
    MMX_HIP(stage.bring(h.oWeight, jb.weight, cnt, k.weight));
    MMX_HIP(stage.bring(h.oProjection, jb.type == MMX_JC_PROJECTION ? jb.projection : nullptr, 12 * cnt, k.projection));
  }
  MMX_HIP(stage.finish()); // the caller may free its host arrays on return
  // ---- the descriptors, from the record
  pb->tablesDirty = pb->tablesDirty || in.structureChanged;
  pb->ellipsoids.assign(c->ellipsoid_limits, c->ellipsoid_limits + c->num_ellipsoid_limits);
  pb->limits = std::move(in.limits);
  pb->genRows = in.genRows;
  pb->M = in.M;
  static_assert(sizeof(mmx_parameter_limit) == sizeof(mmx::LimitDev) && sizeof(mmx::LimitDev) == 32, "limit layouts must match");
  MMX_HIP(upload(pb->dLimits, pb->limits));
  d.NL = int32_t(pb->limits.size());
  d.limits = pb->dLimits.as<mmx::LimitDev>();
  d.fnCols = in.fnCols;
  d.wPos = c->pos_function_weight;
  d.wOri = c->ori_function_weight;
  d.wLimit = c->limit_function_weight;
  d.wModel = c->model_function_weight;
  d.lossPos = lossDev(in.lossPos);
  d.lossOri = lossDev(in.lossOri);
  d.hasModel = in.hasModel ? 1 : 0;
  d.M = in.M;
  d.rowsJoint = in.rowsJoint;
  // ---- the tables
  if (in.structureChanged) { // the fused kernel's solve list and limit tables depend on it
    MMX_TRY(uploadProblemTables(pb));
    pb->tablesDirty = false;
  } else { // payload pointers / weights / losses of the blocks may still have changed
    MMX_HIP(upload(pb->dBlocks, pb->blockDev));
    d.blocks = pb->dBlocks.as<mmx::JointBlockDev>();
  }
  pb->haveConstraints = true;
  return MMX_OK;
}

int32_t mmx_eval_jacobian(
    mmx_problem* pb,
    const float* theta_dev,
    float* jac_dev,
    float* res_dev,
    double* err_dev,
    int32_t layout,
    void* stream) {
  MMX_ZONE("mmx_eval_jacobian (initializeJacobianComputation + computeJacobianBlock)");
  MMX_TRY(checkProblem(pb, true));
  if (theta_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta is null");
  }
  if (layout != MMX_LAYOUT_COL_MAJOR && layout != MMX_LAYOUT_ROW_MAJOR) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "unknown Jacobian layout");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (layout == MMX_LAYOUT_ROW_MAJOR && jac_dev != nullptr) {
    // assembled column-major (the layout the kernel's coalesced column stores are built for) into the
    // problem's scratch, then transposed per instance: one extra read + write of J
    MMX_HIP(pb->sJacColMajor.ensure(size_t(pb->B) * size_t(pb->M) * size_t(pb->rig->P) * sizeof(float)));
    MMX_HIP(mmx::launchFkJacobian(pb->rigDev, pb->dev, theta_dev, pb->sJacColMajor.as<float>(), res_dev, err_dev, nullptr, nullptr, s));
    MMX_HIP(mmx::launchTransposeJacobian(pb->sJacColMajor.as<float>(), jac_dev, pb->B, pb->M, pb->rig->P, s));
    return MMX_OK;
  }
  MMX_HIP(mmx::launchFkJacobian(pb->rigDev, pb->dev, theta_dev, jac_dev, res_dev, err_dev, nullptr, nullptr, s));
  return MMX_OK;
}

int32_t mmx_eval_jacobian_timed(
    mmx_problem* pb,
    const float* theta_dev,
    float* jac_dev,
    float* res_dev,
    double* err_dev,
    int32_t layout,
    void* stream,
    float* kernel_ms) {
  MMX_TRY(checkProblem(pb, true));
  if (theta_dev == nullptr || jac_dev == nullptr || kernel_ms == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta / jac / kernel_ms is null");
  }
  if (layout != MMX_LAYOUT_COL_MAJOR) {
    return fail(MMX_ERR_UNSUPPORTED, "only MMX_LAYOUT_COL_MAJOR (the reference's layout) is implemented");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  MMX_HIP(hipEventCreate(&e0));
  hipError_t err = hipEventCreate(&e1);
  if (err == hipSuccess) {
    err = mmx::launchFkJacobian(
        pb->rigDev, pb->dev, theta_dev, jac_dev, res_dev, err_dev, nullptr, nullptr, static_cast<hipStream_t>(stream), e0, e1);
  }
  if (err == hipSuccess) {
    err = hipEventSynchronize(e1);
  }
  if (err == hipSuccess) {
    err = hipEventElapsedTime(kernel_ms, e0, e1);
  }
  (void)hipEventDestroy(e0);
  if (e1 != nullptr) {
    (void)hipEventDestroy(e1);
  }
  MMX_HIP(err);
  return MMX_OK;
}

int32_t mmx_debug_store_pattern(mmx_problem* pb, float* jac_dev, void* stream, float* kernel_ms) {
  MMX_TRY(checkProblem(pb, true));
  if (jac_dev == nullptr || kernel_ms == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "jac / kernel_ms is null");
  }
  if (pb->dev.M != pb->dev.rowsJoint || pb->dev.M != 3 * pb->dev.U) {
    return fail(MMX_ERR_UNSUPPORTED, "store pattern: position / orientation rows only");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  MMX_HIP(hipEventCreate(&e0));
  hipError_t err = hipEventCreate(&e1);
  if (err == hipSuccess) {
    err = mmx::launchStorePattern(jac_dev, pb->B, pb->dev.M, pb->rig->dev.P, mmx::fkJacobianWavesPerInstance(pb->rigDev, pb->dev, true), static_cast<hipStream_t>(stream), e0, e1);
  }
  if (err == hipSuccess) {
    err = hipEventSynchronize(e1);
  }
  if (err == hipSuccess) {
    err = hipEventElapsedTime(kernel_ms, e0, e1);
  }
  (void)hipEventDestroy(e0);
  if (e1 != nullptr) {
    (void)hipEventDestroy(e1);
  }
  MMX_HIP(err);
  return MMX_OK;
}

int32_t mmx_eval_skeleton_state(mmx_problem* pb, const float* theta_dev, float* state_dev, void* stream) {
  MMX_ZONE("mmx_eval_skeleton_state (SkeletonState::set)");
  MMX_TRY(checkProblem(pb, false));
  if (theta_dev == nullptr || state_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta / state is null");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(mmx::launchFkJacobian(
      pb->rigDev, pb->dev, theta_dev, nullptr, nullptr, nullptr, state_dev, nullptr, static_cast<hipStream_t>(stream), nullptr, nullptr, true));
  return MMX_OK;
}

namespace {
int32_t ensureStepScratch(mmx_problem* pb, bool needJacobian = true) {
  const size_t B = size_t(pb->B), M = size_t(pb->M), P = size_t(pb->rig->P), n = size_t(pb->dev.n);
  if (needJacobian) {
    MMX_HIP(pb->sJac.ensure(B * M * P * sizeof(float)));
  }
  MMX_HIP(pb->sRes.ensure(B * std::max<size_t>(M, 1) * sizeof(float)));
  MMX_HIP(pb->sErr.ensure(B * sizeof(double)));
  MMX_HIP(pb->sJtj.ensure(B * n * n * sizeof(float)));
  MMX_HIP(pb->sJtr.ensure(B * n * sizeof(float)));
  return MMX_OK;
}
} // namespace

int32_t mmx_eval_normal_equations(
    mmx_problem* pb,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    double* err_dev,
    void* stream) {
  MMX_ZONE("mmx_eval_normal_equations (Get JtJ and JtR)");
  MMX_TRY(checkProblem(pb, true));
  if (theta_dev == nullptr || jtj_dev == nullptr || jtr_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta / jtj / jtr is null");
  }
  if (pb->dev.n > mmx::kMaxSolved) {
    return fail(MMX_ERR_UNSUPPORTED, "more than 2048 enabled parameters (kMaxModelParams)");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  MMX_TRY(ensureStepScratch(pb));
  MMX_HIP(mmx::launchFkJacobian(
      pb->rigDev, pb->dev, theta_dev, pb->sJac.as<float>(), pb->sRes.as<float>(), err_dev, nullptr, nullptr, s));
  MMX_HIP(mmx::launchNormalEquations(
      pb->dev, pb->rig->P, pb->sJac.as<float>(), pb->sRes.as<float>(), jtj_dev, jtr_dev, nullptr, false, s));
  return MMX_OK;
}

int32_t mmx_debug_tree_normal_equations(mmx_problem* pb, const float* theta_dev, float* jtj_dev, float* jtr_dev, void* stream) {
  MMX_ZONE("mmx_debug_tree_normal_equations");
  MMX_TRY(checkProblem(pb, true));
  if (theta_dev == nullptr || jtj_dev == nullptr || jtr_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta / jtj / jtr is null");
  }
  if (!treeNormalEquationsUsable(pb) || pb->solveN != pb->dev.n) {
    return fail(MMX_ERR_UNSUPPORTED, "mmx_debug_tree_normal_equations: problem outside the tree-moment kernel's scope (or structurally zero columns present)");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  MMX_HIP(mmx::zeroAsync(jtj_dev, size_t(pb->B) * size_t(pb->dev.n) * size_t(pb->dev.n) * sizeof(float), s));
  const SolveView sv = solveView(pb);
  MMX_HIP(mmx::launchTreeNormalEquations(sv.rig, sv.pb, sv.fd, theta_dev, jtj_dev, jtr_dev, nullptr, nullptr, nullptr, nullptr, nullptr, false, s));
  return MMX_OK;
}

int32_t mmx_problem_solve_diagnostics(mmx_problem* pb, float* diag_dev, void* stream) {
  MMX_TRY(checkProblem(pb, true));
  if (diag_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "diag_dev is null");
  }
  if (!pb->diagValid) {
    return fail(MMX_ERR_UNSUPPORTED, "mmx_problem_solve_diagnostics: no single-precision solve on the one-launch or wide route has run on this handle");
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(hipMemcpyAsync(diag_dev, pb->sDiag.p, size_t(pb->B) * 4 * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return MMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The solve dispatch.  An entry point checks its handle and pointers, gathers the facts the decision reads (solveFacts), asks
// mmx_solve_plan.cpp for the plan and either fails with the plan's refusal -- before theta, an output, lastRoute or diagValid
// is touched -- or runs the plan's stages: one executor per route and precision below, on the shared set-up blocks.
extern "C++" {
namespace {

static_assert(mmx::kPlanMaxSolved == mmx::kMaxSolved, "the solve plan's bound is the kernels'");

// the optional outputs of a solve, as the caller passed them (null: not wanted)
struct SolveOutputs {
  double* finalError;
  int32_t* iterations;
  int32_t* status;
  double* errorHistory;
  float* parameterHistory;
  double* stepHistory;
};

// What the plan reads, gathered in one place.  The sizing functions stay with their kernels.  The budgets of kernels the call
// cannot reach are left at their defaults: the wave route's unless it is pinned or asked for (mmx_solve_frames), the mixed and
// double kernels' under MMX_PRECISION_F32 (mmx_solve_f64 passes another precision).
mmx::SolveFacts solveFacts(const mmx_problem* pb, const SolveOutputs& out, int32_t precision, bool wave) {
  const mmx::ProblemDev& d = pb->dev;
  const int J = pb->rig->J, P = pb->rig->P, U = pb->U, n = pb->fdev.n;
  mmx::SolveFacts f;
  f.route = pb->tuning.route;
  f.refineSteps = refineSteps(pb);
  f.fusedUsable = fusedUsable(pb);
  f.treeUsable = treeNormalEquationsUsable(pb);
  f.fusedBlocks = mmx::fusedBlocksFor(n);
  f.choleskyStepLdsBytes = mmx::choleskyStepLdsBytes(pb->solveN, d.M);
  if (wave) {
    f.waveLdsBytes = mmx::waveLdsBytes(J, P, U, n, false);
    f.waveFramesLdsBytes = mmx::waveLdsBytes(J, P, U, n, true);
  }
  if (precision != MMX_PRECISION_F32) {
    const int genRowsF64 = d.rowsJoint - 3 * U;
    f.fusedMixedUsable = mmx::fusedMixedUsable(J, P, U, pb->fdev.nsrc, n, pb->fdev.numCells);
    f.f64Resident = mmx::solveF64IsResident(J, P, U, pb->solveN, d.G + d.NE, genRowsF64);
    f.f64LdsBytes = mmx::solveF64LdsBytes(J, P, U, pb->solveN, d.G + d.NE, genRowsF64);
  }
  f.J = J;
  f.n = n;
  f.solveN = pb->solveN;
  f.U = U;
  f.M = d.M;
  f.rowsJoint = d.rowsJoint;
  f.GT = pb->fdev.GT;
  f.G = d.G;
  f.NE = d.NE;
  f.NL = d.NL;
  f.numBlocks = d.numBlocks;
  f.hasModel = d.hasModel;
  f.lossPosType = d.lossPos.type;
  f.lossOriType = d.lossOri.type;
  f.instanceParents = d.instPosParent != nullptr || d.instOriParent != nullptr;
  f.parameterHistory = out.parameterHistory != nullptr;
  f.stepHistory = out.stepHistory != nullptr;
  return f;
}

// ---- the set-up blocks every executor shares

// The three default output buffers, and the solve state with the caller's pointers or the defaults
int32_t bindOutputs(mmx_problem* pb, const SolveOutputs& out, mmx::SolveStateDev& st) {
  const size_t B = size_t(pb->B);
  MMX_HIP(pb->sIters.ensure(B * sizeof(int32_t)));
  MMX_HIP(pb->sStatus.ensure(B * sizeof(int32_t)));
  MMX_HIP(pb->sFinalErr.ensure(B * sizeof(double)));
  st = mmx::SolveStateDev{};
  st.iterations = out.iterations != nullptr ? out.iterations : pb->sIters.as<int32_t>();
  st.status = out.status != nullptr ? out.status : pb->sStatus.as<int32_t>();
  st.finalError = out.finalError != nullptr ? out.finalError : pb->sFinalErr.as<double>();
  st.errorHistory = out.errorHistory;
  st.paramHistory = out.parameterHistory;
  st.stepHistory = out.stepHistory;
  return MMX_OK;
}

// ... with the [B][4] diagnostics of the one-launch instantiations
int32_t bindDiagnostics(mmx_problem* pb, const mmx_gn_options* o, mmx::SolveStateDev& st) {
  MMX_HIP(pb->sDiag.ensure(size_t(pb->B) * 4 * sizeof(float)));
  st.diag = pb->sDiag.as<float>();
  st.precisionBound = o->precision_bound > 0.f ? o->precision_bound : 1e-5f;
  pb->diagValid = true;
  return MMX_OK;
}

// Zeroes the histories that were passed (rows past an element's last iteration stay zero): step, error, parameters
int32_t zeroHistories(const mmx_problem* pb, const mmx_gn_options* o, const SolveOutputs& out, hipStream_t s) {
  const size_t rows = size_t(pb->B) * size_t(std::max(o->max_iterations, 0));
  if (out.stepHistory != nullptr && rows > 0) {
    MMX_HIP(mmx::zeroAsync(out.stepHistory, rows * 2 * sizeof(double), s));
  }
  if (out.errorHistory != nullptr && rows > 0) {
    MMX_HIP(mmx::zeroAsync(out.errorHistory, rows * sizeof(double), s));
  }
  if (out.parameterHistory != nullptr && rows > 0) {
    MMX_HIP(mmx::zeroAsync(out.parameterHistory, rows * size_t(pb->rig->P) * sizeof(float), s));
  }
  return MMX_OK;
}

// mmx_gn_options as the one-launch kernels take them.  The mixed and double executors overwrite what differs by design; the
// wave launcher reads lambda, threshold, the iteration counts, refine and doLineSearch only (launchWave, mmx_wave.hip).
mmx::FusedParams fusedParams(const mmx_problem* pb, const mmx_gn_options* o) {
  mmx::FusedParams fp{};
  fp.lambda = o->regularization;
  fp.threshold = o->threshold;
  fp.minIterations = o->min_iterations;
  fp.maxIterations = o->max_iterations;
  fp.refine = refineSteps(pb);
  fp.doLineSearch = o->do_line_search;
  fp.stepRule = o->step_rule;
  fp.lmLambdaMin = o->lm_lambda_min;
  fp.lmLambdaMax = o->lm_lambda_max;
  fp.lmUp = o->lm_up;
  fp.lmDown = o->lm_down;
  fp.trustRadius = o->trust_region_radius > 0.f ? o->trust_region_radius : 1.f;
  return fp;
}

// Profiling aid (MMX_PHASE_CLOCKS): per-phase cycles of block 0.  armPhaseClocks leaves *clk null when they are not wanted;
// printPhaseClocks reads them back (it synchronises the stream) and prints `count` rows under their names, with their share of
// `total` when that is not negative.
int32_t armPhaseClocks(mmx_problem* pb, bool withStop, hipStream_t s, long long** clk) {
  *clk = nullptr;
  if (!phaseClocksWanted()) {
    return MMX_OK;
  }
  MMX_HIP(pb->sClk.ensure(32 * sizeof(long long)));
  MMX_HIP(hipMemsetAsync(pb->sClk.p, 0, 32 * sizeof(long long), s));
  *clk = pb->sClk.as<long long>();
  if (withStop) {
    MMX_HIP(armPhaseStop(*clk, s));
  }
  return MMX_OK;
}

int32_t readPhaseClocks(const long long* clk, hipStream_t s, long long (&h)[32]) {
  MMX_HIP(hipMemcpyAsync(h, clk, sizeof(h), hipMemcpyDeviceToHost, s));
  MMX_HIP(hipStreamSynchronize(s));
  return MMX_OK;
}

void printPhaseClocks(const char* const* names, int count, int width, const long long* h, long long total) {
  for (int i = 0; i < count; ++i) {
    if (total < 0) {
      fprintf(stderr, "  %-*s %10lld\n", width, names[i], h[i]);
    } else {
      fprintf(stderr, "  %-*s %10lld  %5.1f%%\n", width, names[i], h[i], 100.0 * double(h[i]) / double(total > 0 ? total : 1));
    }
  }
}

// ---- the executors: one per route of a single-precision stage, the mixed instantiation, the double kernel

// MMX_ROUTE_WAVE: one wavefront per instance, the whole SolverT::solve loop in one launch (small rigs); numFrames > 0: one
// wavefront per sequence (mmx_solve_frames).  No precision estimate on this route.
int32_t runWave(mmx_problem* pb, const mmx_gn_options* o, float* theta_dev, const SolveOutputs& out, int32_t numFrames, hipStream_t s) {
  pb->lastRoute = MMX_ROUTE_WAVE;
  pb->diagValid = false;
  mmx::SolveStateDev wst;
  MMX_TRY(bindOutputs(pb, out, wst));
  MMX_TRY(zeroHistories(pb, o, out, s));
  const mmx::FusedParams wp = fusedParams(pb, o);
  const SolveView sv = solveView(pb);
  if (numFrames > 0) {
    MMX_HIP(mmx::launchWaveFrames(sv.rig, sv.pb, sv.fd, theta_dev, wst, wp, numFrames, s));
    return MMX_OK;
  }
  MMX_ZONE("wave solve: all iterations in one launch, one wavefront per instance");
  MMX_HIP(mmx::launchWaveSolve(sv.rig, sv.pb, sv.fd, theta_dev, wst, wp, s));
  return MMX_OK;
}

// MMX_ROUTE_FUSED: the whole SolverT::solve loop in one launch, one workgroup per instance
int32_t runFused(mmx_problem* pb, const mmx_gn_options* o, const mmx::SolveStage& stage, float* theta_dev, const SolveOutputs& out, hipStream_t s) {
  pb->lastRoute = MMX_ROUTE_FUSED;
  mmx::SolveStateDev fst;
  MMX_TRY(bindOutputs(pb, out, fst));
  MMX_TRY(bindDiagnostics(pb, o, fst));
  MMX_TRY(zeroHistories(pb, o, out, s));
  mmx::FusedParams fp = fusedParams(pb, o);
  fp.autoAbort = stage.mayAbort ? 1 : 0;
  long long* clk = nullptr;
  MMX_TRY(armPhaseClocks(pb, true, s, &clk));
  {
    MMX_ZONE("fused solve: all iterations of GaussNewtonSolverT::doIteration in one launch");
    MMX_HIP(pb->sFusedArgs.ensure(mmx::fusedArgsBytes()));
    const SolveView sv = solveView(pb);
    MMX_HIP(mmx::launchFusedSolve(sv.rig, sv.pb, sv.fd, theta_dev, fst, fp, nullptr, nullptr, clk, pb->sFusedArgs.p, s));
  }
  if (clk != nullptr) {
    long long h[32];
    MMX_TRY(readPhaseClocks(clk, s, h));
    static const char* names[24] = {"A jointParams", "B fk", "C units", "D subtree sums", "E srcTables", "F g + zero tiles",
                                    "G combine + pull", "H cholesky(tail)", "I solve", "J tail (d0 += rho)", "K update",
                                    "G extras: records", "G term records", "H.bc panel", "H.d mfma", "D own sums", "J jd",
                                    "J tangent+own", "J subtree", "J rho", "J solve", "G extras: loads", "H.b load+barrier", "H.b chain"};
    const long long tot = std::accumulate(h, h + 27, 0LL);
    fprintf(stderr, "[mmx phase clocks, block 0, all iterations] total %lld  (termRounds %d, numComb %d, nsrc %d, n %d)\n", tot, pb->fdev.termRounds, pb->fdev.numComb, pb->fdev.nsrc, pb->fdev.n);
    printPhaseClocks(names, 24, 16, h, tot);
    fprintf(stderr, "  (of B fk: joint parameters %lld, local transforms %lld, pointer jumping %lld, axes = the rest of B)\n", h[26], h[24], h[25]);
  }
  return MMX_OK;
}

// The mixed-precision instantiation of the one-launch solve (MMX_PRECISION_MIXED, MMX_PRECISION_AUTO's second stage).  An
// escalation stage (sel.map set) leaves the single-precision stage's histories and diagnostics for the other elements.
int32_t runMixed(mmx_problem* pb, const mmx_gn_options* o, float* theta_dev, const SolveOutputs& out, const mmx::MixSelect& sel, hipStream_t s) {
  MMX_ZONE("mmx_solve, mixed precision (SolverT<double>::solve around a single-precision factor)");
  pb->lastRoute = MMX_ROUTE_FUSED;
  mmx::SolveStateDev fst;
  MMX_TRY(bindOutputs(pb, out, fst));
  if (sel.map == nullptr) {
    MMX_TRY(bindDiagnostics(pb, o, fst));
    MMX_TRY(zeroHistories(pb, o, out, s));
  }
  fst.precisionBound = o->precision_bound > 0.f ? o->precision_bound : 1e-5f;
  mmx::FusedParams fp = fusedParams(pb, o);
  fp.refine = 0;
  fp.trustRadius = 1.f;
  fp.mixTol = pb->tuning.mixed_tolerance > 0.f ? pb->tuning.mixed_tolerance : 3e-9f;
  fp.mixMaxCg = pb->tuning.mixed_max_cg > 0 ? pb->tuning.mixed_max_cg : 12;
  long long* clk = nullptr;
  MMX_TRY(armPhaseClocks(pb, true, s, &clk));
  const SolveView sv = solveView(pb);
  MMX_HIP(mmx::launchFusedMixed(sv.rig, sv.pb, sv.fd, theta_dev, fst, fp, sel, pb->B, clk, s));
  if (clk != nullptr) {
    long long h[32];
    MMX_TRY(readPhaseClocks(clk, s, h));
    static const char* names[24] = {"-", "A-C fk + units (double)", "(reused state)", "D subtree sums", "E srcTables", "F g (double adjoint)",
                                    "G combine + pull", "H cholesky(tail)", "-", "-", "K update",
                                    "G extras: records", "G term records", "H.bc panel", "H.d mfma", "D own sums", "CG z0 solve + rz",
                                    "CG operator (double)", "CG decide + direction", "CG dots + update", "CG solve", "G extras: loads", "H.b load+barrier", "H.b chain"};
    const long long tot = std::accumulate(h, h + 24, 0LL);
    fprintf(stderr, "[mmx phase clocks, MIXED, block 0, all iterations] total %lld\n", tot);
    printPhaseClocks(names, 24, 26, h, tot);
  }
  return MMX_OK;
}

// mmx::F64AssemblyList for chunks of `uc` units (mmx::buildF64AssemblyListHost), uploaded
int32_t buildF64AssemblyList(mmx_problem* pb, int32_t uc) {
  mmx::F64AssemblyListHost h;
  if (!mmx::buildF64AssemblyListHost(pb->tables, pb->solveListF64, pb->posParent.data(), pb->Kp, pb->oriParent.data(), pb->Ko, uc, h)) {
    return fail(MMX_ERR_UNSUPPORTED, "mmx_solve_f64: more than 8191 sources of one column apply to one constraint");
  }
  if (h.groups.empty()) {
    h.groups.assign(2, 0u);
  }
  if (h.extra.empty()) {
    h.extra.push_back(0);
  }
  MMX_HIP(upload(pb->dF64Groups, h.groups));
  MMX_HIP(upload(pb->dF64Extra, h.extra));
  MMX_HIP(upload(pb->dF64ChunkStart, h.chunkStart));
  pb->f64ListUnitsPerChunk = uc;
  return MMX_OK;
}

bool residentF64(const mmx_problem* pb) {
  return mmx::solveF64IsResident(pb->rig->J, pb->rig->P, pb->U, pb->solveN, pb->dev.G + pb->dev.NE, pb->dev.rowsJoint - 3 * pb->U);
}

// The scratch form of the double kernel: dense J and H of every element in a global scratch of the problem.  MMX_PRECISION_AUTO
// allocates it before its single-precision stage, so that a failure of the later stage leaves the caller's arrays untouched.
int32_t ensureF64Scratch(mmx_problem* pb) {
  const size_t B = size_t(pb->B), n = size_t(pb->solveN), M = size_t(pb->dev.rowsJoint);
  if (!residentF64(pb)) {
    MMX_HIP(pb->sJacF64.ensure(std::max<size_t>(B * n * M, 1) * sizeof(double)));
    MMX_HIP(pb->sHessF64.ensure(std::max<size_t>(B * n * n, 1) * sizeof(double)));
  }
  return MMX_OK;
}

// The double instantiation (mmx_solve_f64; MMX_PRECISION_F64 and the last stage of MMX_PRECISION_AUTO of mmx_solve).
// theta_dev: double [B][P] in / out, or null when `select` carries float arrays.  It records no route, and no parameter
// history (the plan refuses a call that passes one); an escalation stage (select.map set) leaves the earlier stages' histories for the other elements.
int32_t runDouble(mmx_problem* pb, const mmx_gn_options* o, double* theta_dev, const SolveOutputs& out, const mmx::F64Select& select, hipStream_t s) {
  MMX_ZONE("mmx_solve_f64 (SolverT<double>::solve)");
  const size_t B = size_t(pb->B), n = size_t(pb->solveN);
  const int genRowsF64 = pb->dev.rowsJoint - 3 * pb->U;
  MMX_TRY(ensureF64Scratch(pb));
  const bool trustF64 = o->step_rule == MMX_STEP_TRUST_REGION;
  if (trustF64) {
    MMX_HIP(pb->sHess2F64.ensure(std::max<size_t>(B * n * n, 1) * sizeof(double)));
  }
  mmx::SolveStateDev st;
  MMX_TRY(bindOutputs(pb, out, st));
  if (select.map == nullptr && o->max_iterations > 0) { // (this path zeroes the error history first and records no parameter history)
    const size_t rows = B * size_t(o->max_iterations);
    if (out.errorHistory != nullptr) {
      MMX_HIP(mmx::zeroAsync(out.errorHistory, rows * sizeof(double), s));
    }
    if (out.stepHistory != nullptr) {
      MMX_HIP(mmx::zeroAsync(out.stepHistory, rows * 2 * sizeof(double), s));
    }
  }
  mmx::FusedParams fp = fusedParams(pb, o);
  fp.refine = 0;
  mmx::F64AssemblyList alist{nullptr, nullptr, nullptr, 0};
  if (residentF64(pb) && pb->dev.instPosParent == nullptr && pb->dev.instOriParent == nullptr && pb->rig->J < 4096 && pb->solveN <= 4096) {
    const int32_t uc = mmx::solveF64ResidentChunkRows(pb->rig->J, pb->rig->P, pb->U, pb->solveN, pb->dev.G + pb->dev.NE, genRowsF64) / 3;
    if (uc > 0 && uc <= 64) {
      if (pb->f64ListUnitsPerChunk != uc) {
        MMX_TRY(buildF64AssemblyList(pb, uc));
      }
      alist = mmx::F64AssemblyList{pb->dF64Groups.as<uint2>(), pb->dF64Extra.as<int32_t>(), pb->dF64ChunkStart.as<int32_t>(), uc};
    }
  }
  MMX_HIP(mmx::launchSolveF64(
      pb->rigDev, pb->dev, pb->dSolveListF64.as<int32_t>(), pb->solveN, theta_dev, st, fp, pb->sJacF64.as<double>(), pb->sHessF64.as<double>(), trustF64 ? pb->sHess2F64.as<double>() : nullptr, s, alist, select));
  return MMX_OK;
}

// ---- the host-driven routes (MMX_ROUTE_WIDE, MMX_ROUTE_EXPLICIT_JACOBIAN): several kernels per iteration

struct HostDriven {
  mmx::ProblemDev ds; // the explicit-Jacobian solver's view: structurally zero columns dropped
  mmx::SolveStateDev st;
  mmx::StepParams sp;
  float* factorScratch = nullptr; // wide systems: the left-looking Cholesky step keeps L in its own tile-major scratch
  float* genState = nullptr; // J_g of the further joint error functions / ellipsoid limits, tree kernels' hand-over
  SolveView sv; // (the tree kernels' descriptors; everything else on these routes keeps the full rig)
};

// Scratch, solve state and step parameters of a host-driven solve; the initial parameters are kept for the finalize kernel
int32_t prepareHostDriven(
    mmx_problem* pb, const mmx_gn_options* o, const mmx::SolveStage& stage, const float* theta_dev, const SolveOutputs& out, hipStream_t s, HostDriven& hd) {
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P);
  const bool trust = o->step_rule == MMX_STEP_TRUST_REGION;
  hd.ds = pb->dev;
  hd.ds.n = pb->solveN;
  hd.ds.enabledList = pb->dSolveListV1.as<int32_t>();
  const int n = hd.ds.n;
  MMX_TRY(ensureStepScratch(pb, !stage.treeRefine));
  MMX_HIP(pb->sThetaInit.ensure(B * P * sizeof(float)));
  MMX_HIP(pb->sDone.ensure(B * sizeof(int32_t)));
  MMX_HIP(pb->sLastErr.ensure(B * sizeof(double)));
  SolveOutputs bound = out;
  bound.parameterHistory = nullptr; // (copied after every iteration and finalised: iterateHostDriven, runHostDriven)
  mmx::SolveStateDev& st = hd.st;
  MMX_TRY(bindOutputs(pb, bound, st));
  st.done = pb->sDone.as<int32_t>();
  st.lastError = pb->sLastErr.as<double>();
  pb->diagValid = false; // (the wide route's estimate: below)
  MMX_TRY(zeroHistories(pb, o, bound, s));
  MMX_HIP(hipMemcpyAsync(pb->sThetaInit.p, theta_dev, B * P * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (stage.deferred) {
    MMX_HIP(pb->sDelta.ensure(B * size_t(std::max(n, 1)) * sizeof(float)));
    MMX_HIP(pb->sStepIter.ensure(B * sizeof(int32_t)));
    MMX_HIP(mmx::zeroAsync(pb->sStepIter.p, B * sizeof(int32_t), s));
  }
  if (stage.schedule) {
    MMX_HIP(pb->sLambda.ensure(B * sizeof(float)));
  }
  if (stage.wideDiag) { // the precision estimate on the wide route (tree kernels + tile factor + finish stage)
    MMX_HIP(pb->sDiagAcc.ensure(B * 4 * sizeof(float)));
    MMX_HIP(pb->sDiagErr0.ensure(B * sizeof(float)));
    MMX_TRY(bindDiagnostics(pb, o, st));
  }
  MMX_HIP(mmx::launchSolveInit(st, pb->B, stage.schedule ? pb->sLambda.as<float>() : nullptr, o->regularization, s, stage.wideDiag ? pb->sDiagAcc.as<float>() : nullptr));
  mmx::StepParams& sp = hd.sp;
  sp = mmx::StepParams{};
  sp.diagAcc = stage.wideDiag ? pb->sDiagAcc.as<float>() : nullptr;
  sp.diagErr0 = stage.wideDiag ? pb->sDiagErr0.as<float>() : nullptr;
  sp.lambda = o->regularization;
  sp.threshold = o->threshold;
  sp.minIterations = o->min_iterations;
  sp.maxIterations = o->max_iterations;
  sp.refine = refineSteps(pb);
  sp.tileMasks = pb->dTileMasks.as<uint32_t>();
  sp.numTiles = int32_t(pb->tileMasks.tiles.size());
  sp.delta = stage.deferred ? pb->sDelta.as<float>() : nullptr;
  sp.stepIter = stage.deferred ? pb->sStepIter.as<int32_t>() : nullptr;
  sp.lambdaPer = stage.schedule ? pb->sLambda.as<float>() : nullptr;
  sp.stepHistory = out.stepHistory;
  sp.doLineSearch = trust ? 0 : o->do_line_search; // (the trust region reads neither do_line_search nor regularization)
  sp.stepRule = o->step_rule;
  if (trust) {
    MMX_HIP(pb->sTrust.ensure(B * 6 * sizeof(int32_t) + 16));
    char* base = static_cast<char*>(pb->sTrust.p);
    sp.tr.lambda = reinterpret_cast<float*>(base);
    sp.tr.radius = reinterpret_cast<float*>(base + B * 4);
    sp.tr.phase = reinterpret_cast<int32_t*>(base + B * 8);
    sp.tr.newton = reinterpret_cast<int32_t*>(base + B * 12);
    sp.tr.step = reinterpret_cast<int32_t*>(base + B * 16);
    sp.tr.mask = reinterpret_cast<int32_t*>(base + B * 20);
    sp.tr.active = reinterpret_cast<int32_t*>(base + B * 24);
    MMX_HIP(mmx::launchTrustInit(sp.tr, pb->B, o->trust_region_radius > 0.f ? o->trust_region_radius : 1.f, s));
  }
  sp.lmLambdaMin = o->lm_lambda_min;
  sp.lmLambdaMax = o->lm_lambda_max;
  sp.lmUp = o->lm_up;
  sp.lmDown = o->lm_down;
  MMX_TRY(armPhaseClocks(pb, false, s, &sp.clk));
  if (stage.wide || stage.treeRefine) {
    MMX_HIP(pb->sFactor.ensure(B * mmx::choleskyFactorFloats(n) * sizeof(float)));
    hd.factorScratch = pb->sFactor.as<float>();
  }
  if (stage.treeRefine) {
    // (H travels tile-major on this route: NB (NB + 1) / 2 tiles of 256 floats, more than n^2 for small systems)
    const size_t NPs = (size_t(n) + 15) & ~size_t(15);
    MMX_HIP(pb->sJtj.ensure(std::max(B * size_t(pb->dev.n) * size_t(pb->dev.n), B * mmx::choleskyFactorFloats(n)) * sizeof(float)));
    MMX_HIP(pb->sTreeState.ensure(B * mmx::treeStateFloats(pb->rig->J, pb->fdev.U) * sizeof(float)));
    MMX_HIP(pb->sDvec.ensure(B * NPs * sizeof(float)));
    MMX_HIP(pb->sRhoVec.ensure(B * NPs * sizeof(float)));
    MMX_HIP(pb->sRefState.ensure(B * sizeof(int32_t)));
    if (pb->fdev.GT > 0) {
      MMX_HIP(pb->sGenState.ensure(B * mmx::treeGenStateFloats(pb->fdev.n, pb->fdev.genRows) * sizeof(float)));
      hd.genState = pb->sGenState.as<float>();
    }
  }
  hd.sv = solveView(pb);
  return MMX_OK;
}

// The wide route's linear solve for the instances `who` leaves in: factor + first solve, then up to three refinement rounds;
// an instance whose correction fell below 1e-3 of its step applies the step and sits out the remaining rounds (its workgroups
// return at once)
int32_t treeLinearSolve(mmx_problem* pb, const HostDriven& hd, const mmx::SolveStateDev& who, float* theta_dev, hipStream_t s) {
  const mmx::StepParams& sp = hd.sp;
  MMX_HIP(mmx::launchCholeskyFactorTiled(
      hd.ds, pb->rig->P, pb->sJtj.as<float>(), pb->sJtr.as<float>(), hd.factorScratch, pb->sDvec.as<float>(), pb->sRefState.as<int32_t>(),
      pb->sErr.as<double>(), theta_dev, who, sp, s));
  for (int round = 0; round < sp.refine; ++round) {
    MMX_HIP(mmx::launchTreeRefine(
        hd.sv.rig, hd.sv.pb, hd.sv.fd, theta_dev, pb->sTreeState.as<float>(), hd.genState, pb->sDvec.as<float>(), pb->sRhoVec.as<float>(), pb->sRefState.as<int32_t>(),
        sp.lambda, sp.lambdaPer, s));
    MMX_HIP(mmx::launchCholeskyFinishTiled(
        hd.ds, pb->rig->P, hd.factorScratch, pb->sDvec.as<float>(), pb->sRhoVec.as<float>(), pb->sRefState.as<int32_t>(), pb->sErr.as<double>(),
        theta_dev, who, sp, round, s));
  }
  return MMX_OK;
}

// TrustRegionQRT::doIteration (trust_region_qr.cpp:52-270) from the host: per pass, the instances whose damping changed factor
// and solve, every instance with a step on the table decides (try it, or a Newton update of lambda first), the ready ones run
// their trial.  At most ten trust steps of up to four solves each; the loop ends as soon as no instance is left in the
// iteration (one 4-byte read-back per pass).
int32_t trustRegionPasses(mmx_problem* pb, const HostDriven& hd, float* theta_dev, hipStream_t s) {
  MMX_ZONE("TrustRegionQR: trust steps");
  const mmx::StepParams& sp = hd.sp;
  MMX_HIP(mmx::launchTrustBegin(sp.tr, hd.st, sp.lambdaPer, pb->B, s));
  mmx::SolveStateDev masked = hd.st;
  masked.done = sp.tr.mask;
  for (int pass = 0; pass < 40; ++pass) {
    MMX_TRY(treeLinearSolve(pb, hd, masked, theta_dev, s));
    MMX_HIP(mmx::launchTrustDecide(hd.ds, hd.factorScratch, pb->sJtr.as<float>(), pb->sErr.as<double>(), hd.st, sp, s));
    MMX_HIP(mmx::zeroAsync(sp.tr.active, sizeof(int32_t), s));
    MMX_HIP(mmx::launchStepUpdate(pb->rigDev, hd.ds, theta_dev, pb->sJtr.as<float>(), pb->sErr.as<double>(), sp, s));
    int32_t active = 0;
    MMX_HIP(hipMemcpyAsync(&active, sp.tr.active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MMX_HIP(hipStreamSynchronize(s));
    if (active == 0) {
      break;
    }
  }
  MMX_HIP(mmx::launchTrustEnd(hd.st, sp, pb->sErr.as<double>(), pb->B, s));
  return MMX_OK;
}

// The iteration loop (solver.cpp:89).  The parameter history is copied after every iteration, every element (rows past an
// element's last iteration are zeroed by the caller's finalize kernel).
int32_t iterateHostDriven(
    mmx_problem* pb, const mmx_gn_options* o, const mmx::SolveStage& stage, HostDriven& hd, float* theta_dev, float* parameter_history, hipStream_t s) {
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P);
  const bool trust = o->step_rule == MMX_STEP_TRUST_REGION;
  const mmx::SolveStateDev& st = hd.st;
  mmx::StepParams& sp = hd.sp;
  for (int it = 0; it < o->max_iterations; ++it) {
    sp.iteration = it;
    MMX_ZONE("GaussNewtonSolverT::doIteration");
    if (stage.treeRefine) {
      {
        MMX_ZONE("Get JtJ and JtR");
        MMX_HIP(mmx::launchTreeNormalEquations(
            hd.sv.rig, hd.sv.pb, hd.sv.fd, theta_dev, pb->sJtj.as<float>(), pb->sJtr.as<float>(), st.done, pb->sErr.as<double>(),
            pb->sTreeState.as<float>(), sp.clk != nullptr ? sp.clk + 8 : nullptr, hd.genState, true, s));
      }
      MMX_ZONE("Dense gauss newton step");
      MMX_TRY(trust ? trustRegionPasses(pb, hd, theta_dev, s) : treeLinearSolve(pb, hd, st, theta_dev, s));
    } else {
      {
        MMX_ZONE("Get JtJ and JtR");
        MMX_HIP(mmx::launchFkJacobian(
            pb->rigDev, pb->dev, theta_dev, pb->sJac.as<float>(), pb->sRes.as<float>(), pb->sErr.as<double>(), nullptr, st.done, s, nullptr, nullptr, true));
        MMX_HIP(mmx::launchNormalEquations(
            hd.ds, pb->rig->P, pb->sJac.as<float>(), pb->sRes.as<float>(), pb->sJtj.as<float>(), pb->sJtr.as<float>(), st.done, stage.wide, s));
      }
      {
        MMX_ZONE("Dense gauss newton step");
        MMX_HIP(mmx::launchCholeskyStep(
            hd.ds, pb->rig->P, pb->sJac.as<float>(), pb->sRes.as<float>(), pb->sJtj.as<float>(), pb->sJtr.as<float>(), pb->sErr.as<double>(),
            theta_dev, st, sp, hd.factorScratch, s));
      }
    }
    if (stage.deferred && !trust) {
      MMX_ZONE("Line search");
      MMX_HIP(mmx::launchStepUpdate(pb->rigDev, hd.ds, theta_dev, pb->sJtr.as<float>(), pb->sErr.as<double>(), sp, s));
    }
    if (parameter_history != nullptr) {
      MMX_HIP(hipMemcpy2DAsync(
          parameter_history + size_t(it) * P, size_t(o->max_iterations) * P * sizeof(float), theta_dev, P * sizeof(float), P * sizeof(float), B,
          hipMemcpyDeviceToDevice, s));
    }
  }
  return MMX_OK;
}

int32_t runHostDriven(mmx_problem* pb, const mmx_gn_options* o, const mmx::SolveStage& stage, float* theta_dev, const SolveOutputs& out, hipStream_t s) {
  pb->lastRoute = stage.route;
  HostDriven hd;
  MMX_TRY(prepareHostDriven(pb, o, stage, theta_dev, out, s, hd));
  MMX_TRY(iterateHostDriven(pb, o, stage, hd, theta_dev, out.parameterHistory, s));
  if (out.parameterHistory != nullptr) {
    MMX_HIP(mmx::launchParamHistoryFinalize(out.parameterHistory, hd.st.iterations, pb->B, o->max_iterations, pb->rig->P, s));
  }
  MMX_HIP(mmx::launchSolveFinalize(theta_dev, pb->sThetaInit.as<float>(), pb->rig->P, hd.st, pb->B, s, hd.sp.diagAcc));
  if (hd.sp.clk != nullptr) {
    long long h[32];
    MMX_TRY(readPhaseClocks(hd.sp.clk, s, h));
    static const char* names[16] = {"load H / fence", "factor (in-HBM: write-back + trailing)", "solve", "refine: w = r - J d", "refine: rho = J^T w", "refine: solve", "factor: panel load (in-HBM)", "factor: panel chain (in-HBM)",
                                    "tree NE: load", "tree NE: A, B forward kinematics", "tree NE: C units + hand-over", "tree NE: D own sums",
                                    "tree NE: D subtree sums", "tree NE: E slot tables", "tree NE: F, G tiles", "tree NE: G extras"};
    fprintf(stderr, "[mmx phase clocks, choleskyStepKernel block 0, all iterations] n = %d\n", hd.ds.n);
    printPhaseClocks(names, stage.treeRefine ? 16 : 8, 40, h, -1);
  }
  return MMX_OK;
}

// ---- a plan's stages, in order

int32_t runPlan(mmx_problem* pb, const mmx_gn_options* o, const mmx::SolvePlan& plan, float* theta_dev, SolveOutputs out, hipStream_t s) {
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P);
  int32_t rc = MMX_OK;
  if (plan.numStages > 1) {
    // MMX_PRECISION_AUTO: the later stages start from the initial parameters and run on the elements the stage before them
    // marked.  Everything that can fail in them is settled before the first stage touches theta, status and the histories.
    MMX_TRY(ensureF64Scratch(pb));
    MMX_HIP(pb->sThetaAuto.ensure(B * P * sizeof(float)));
    MMX_HIP(pb->sAutoMap.ensure(B * sizeof(int32_t)));
    MMX_HIP(pb->sAutoCount.ensure(sizeof(int32_t)));
    MMX_HIP(pb->sStatus.ensure(B * sizeof(int32_t)));
    MMX_HIP(hipMemcpyAsync(pb->sThetaAuto.p, theta_dev, B * P * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (out.status == nullptr) {
      out.status = pb->sStatus.as<int32_t>();
    }
  }
  int32_t* const map = pb->sAutoMap.as<int32_t>();
  int32_t* const count = pb->sAutoCount.as<int32_t>();
  for (int i = 0; i < plan.numStages && rc == MMX_OK; ++i) {
    const mmx::SolveStage& stage = plan.stages[i];
    const bool all = stage.select == mmx::SolveStageSelect::All;
    if (stage.select == mmx::SolveStageSelect::SingleSuspects) {
      // a solve without the estimate (explicit-Jacobian route, the wide route's host-driven trust region): the cue stays the damping floor
      const int32_t mask = MMX_SOLVE_ERROR_MASK | MMX_SOLVE_PRECISION_SUSPECT | (pb->diagValid ? 0 : MMX_SOLVE_DAMPING_FLOORED);
      MMX_HIP(mmx::launchSelectSuspect(out.status, pb->B, mask, map, count, s));
    } else if (stage.select == mmx::SolveStageSelect::MixedSuspects) {
      // the elements whose conjugate gradients ran into the step limit in the mixed stage (the single-precision factor is no
      // preconditioner any more: cond x eps ~ 1 -- BASELINE configs[1] at lambda = 1e-5) or that failed there
      MMX_HIP(mmx::launchSelectSuspect(out.status, pb->B, MMX_SOLVE_ERROR_MASK | MMX_SOLVE_PRECISION_SUSPECT, map, count, s, MMX_SOLVE_MIXED));
    }
    if (stage.kind == mmx::SolveStageKind::Mixed) {
      rc = runMixed(pb, o, theta_dev, out, all ? mmx::MixSelect{nullptr, nullptr, nullptr} : mmx::MixSelect{map, count, pb->sThetaAuto.as<float>()}, s);
    } else if (stage.kind == mmx::SolveStageKind::Double) {
      // every workgroup reads its element's parameters before it writes them: in place on the caller's float array
      rc = runDouble(pb, o, nullptr, out, all ? mmx::F64Select{nullptr, nullptr, theta_dev, theta_dev} : mmx::F64Select{map, count, pb->sThetaAuto.as<float>(), theta_dev}, s);
    } else if (stage.route == MMX_ROUTE_WAVE) {
      rc = runWave(pb, o, theta_dev, out, 0, s);
    } else if (stage.route == MMX_ROUTE_FUSED) {
      rc = runFused(pb, o, stage, theta_dev, out, s);
    } else {
      rc = runHostDriven(pb, o, stage, theta_dev, out, s);
    }
  }
  return rc;
}

// mmx_solve and its variants with histories: mmx_gn_options::precision picks the single-precision routes, the mixed or the
// double instantiation on float parameters, or (MMX_PRECISION_AUTO) one after the other on the elements the one before marked
int32_t solveImpl(mmx_problem* pb, const mmx_gn_options* o, float* theta_dev, const SolveOutputs& out, void* stream) {
  MMX_ZONE("mmx_solve (SolverT::solve)");
  if (o != nullptr) {
    if (const char* why = mmx::preHandleRefusal(*o, out.stepHistory != nullptr)) {
      return fail(MMX_ERR_INVALID_ARGUMENT, why);
    }
  }
  MMX_TRY(checkProblem(pb, true));
  if (o == nullptr || theta_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "options / theta is null");
  }
  const mmx::SolvePlan plan = mmx::planSolve(solveFacts(pb, out, o->precision, pb->tuning.route == MMX_ROUTE_WAVE), *o);
  if (plan.code != MMX_OK) {
    return fail(plan.code, plan.message);
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  return runPlan(pb, o, plan, theta_dev, out, static_cast<hipStream_t>(stream));
}

// The *_host entry points: theta (and the outputs asked for) staged through the problem's scratch around `solve`
template <typename T, typename Solve>
int32_t solveStaged(mmx_problem* pb, T* theta_host, double* final_error_host, int32_t* iterations_host, int32_t* status_host, Solve solve) {
  MMX_TRY(checkProblem(pb, true));
  if (theta_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta is null");
  }
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P);
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(pb->sTheta.ensure(B * P * sizeof(T)));
  MMX_HIP(pb->sIters.ensure(B * sizeof(int32_t)));
  MMX_HIP(pb->sStatus.ensure(B * sizeof(int32_t)));
  MMX_HIP(pb->sFinalErr.ensure(B * sizeof(double)));
  MMX_HIP(hipMemcpy(pb->sTheta.p, theta_host, B * P * sizeof(T), hipMemcpyHostToDevice));
  MMX_TRY(solve(pb->sTheta.as<T>(), pb->sFinalErr.as<double>(), pb->sIters.as<int32_t>(), pb->sStatus.as<int32_t>()));
  MMX_HIP(hipDeviceSynchronize());
  MMX_HIP(hipMemcpy(theta_host, pb->sTheta.p, B * P * sizeof(T), hipMemcpyDeviceToHost));
  if (final_error_host) {
    MMX_HIP(hipMemcpy(final_error_host, pb->sFinalErr.p, B * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (iterations_host) {
    MMX_HIP(hipMemcpy(iterations_host, pb->sIters.p, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  if (status_host) {
    MMX_HIP(hipMemcpy(status_host, pb->sStatus.p, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return MMX_OK;
}

} // namespace
} // extern "C++"

int32_t mmx_solve(
    mmx_problem* pb,
    const mmx_gn_options* o,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    void* stream) {
  return solveImpl(pb, o, theta_dev, SolveOutputs{final_error, iterations, status, error_history, nullptr, nullptr}, stream);
}

int32_t mmx_solve_with_history(
    mmx_problem* pb,
    const mmx_gn_options* o,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    float* parameter_history,
    void* stream) {
  return solveImpl(pb, o, theta_dev, SolveOutputs{final_error, iterations, status, error_history, parameter_history, nullptr}, stream);
}

int32_t mmx_solve_with_step_history(
    mmx_problem* pb,
    const mmx_gn_options* o,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    float* parameter_history,
    double* step_history,
    void* stream) {
  return solveImpl(pb, o, theta_dev, SolveOutputs{final_error, iterations, status, error_history, parameter_history, step_history}, stream);
}

int32_t mmx_solve_f64(
    mmx_problem* pb,
    const mmx_gn_options* o,
    double* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    void* stream) {
  if (theta_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "options / theta is null");
  }
  MMX_TRY(checkProblem(pb, true));
  if (o == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "options / theta is null");
  }
  const SolveOutputs out{final_error, iterations, status, error_history, nullptr, nullptr};
  const mmx::SolvePlan plan = mmx::planSolveF64(solveFacts(pb, out, MMX_PRECISION_F64, false), *o);
  if (plan.code != MMX_OK) {
    return fail(plan.code, plan.message);
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  return runDouble(pb, o, theta_dev, out, mmx::F64Select{nullptr, nullptr, nullptr, nullptr}, static_cast<hipStream_t>(stream));
}

int32_t mmx_problem_f64_form(const mmx_problem* pb, int32_t* resident, int32_t* chunk_rows) {
  if (pb == nullptr || pb->rig == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "problem handle is null");
  }
  mmx_gn_options o;
  mmx_gn_options_default(&o);
  const mmx::SolvePlan plan = mmx::planSolveF64(solveFacts(pb, SolveOutputs{}, MMX_PRECISION_F64, false), o);
  if (plan.code != MMX_OK) {
    return fail(plan.code, plan.message);
  }
  // (the arguments of residentF64 and launchSolveF64)
  const int J = pb->rig->J, P = pb->rig->P, G = pb->dev.G + pb->dev.NE, genRows = pb->dev.rowsJoint - 3 * pb->U;
  const bool res = residentF64(pb);
  if (resident != nullptr) {
    *resident = res ? 1 : 0;
  }
  if (chunk_rows != nullptr) {
    *chunk_rows = res ? mmx::solveF64ResidentChunkRows(J, P, pb->U, pb->solveN, G, genRows) : mmx::solveF64ChunkRows(J, P, pb->U, pb->solveN, G, genRows);
  }
  return MMX_OK;
}

int32_t mmx_debug_fused_normal_equations(
    mmx_problem* pb,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    int32_t* solve_list_host,
    int32_t* num_solved,
    void* stream) {
  MMX_TRY(checkProblem(pb, true));
  const int n = pb->fdev.n;
  if (num_solved != nullptr) {
    *num_solved = n;
  }
  if (solve_list_host != nullptr) {
    std::memcpy(solve_list_host, pb->fused.solveList.data(), sizeof(int32_t) * size_t(n));
  }
  if (theta_dev == nullptr || jtj_dev == nullptr || jtr_dev == nullptr) {
    return MMX_OK; // size query only
  }
  if (!fusedUsable(pb)) {
    return fail(MMX_ERR_UNSUPPORTED, "problem shape outside the fused kernel's instantiations");
  }
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P);
  MMX_HIP(hipSetDevice(pb->rig->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  MMX_HIP(pb->sTheta.ensure(B * P * sizeof(float)));
  MMX_HIP(pb->sIters.ensure(B * sizeof(int32_t)));
  MMX_HIP(pb->sStatus.ensure(B * sizeof(int32_t)));
  MMX_HIP(pb->sFinalErr.ensure(B * sizeof(double)));
  MMX_HIP(hipMemcpyAsync(pb->sTheta.p, theta_dev, B * P * sizeof(float), hipMemcpyDeviceToDevice, s));
  mmx::SolveStateDev fst{};
  fst.iterations = pb->sIters.as<int32_t>();
  fst.status = pb->sStatus.as<int32_t>();
  fst.finalError = pb->sFinalErr.as<double>();
  mmx::FusedParams fp{};
  fp.lambda = 0.05f;
  fp.threshold = 1.f;
  fp.minIterations = 1;
  fp.maxIterations = 1;
  fp.refine = 0;
  const SolveView sv = solveView(pb);
  MMX_HIP(mmx::launchFusedSolve(sv.rig, sv.pb, sv.fd, pb->sTheta.as<float>(), fst, fp, jtj_dev, jtr_dev, nullptr, nullptr, s));
  return MMX_OK;
}

int32_t mmx_solve_host(
    mmx_problem* pb,
    const mmx_gn_options* o,
    float* theta_host,
    double* final_error_host,
    int32_t* iterations_host,
    int32_t* status_host) {
  MMX_ZONE("mmx_solve_host");
  return solveStaged<float>(pb, theta_host, final_error_host, iterations_host, status_host, [&](float* theta, double* err, int32_t* iters, int32_t* status) {
    return mmx_solve(pb, o, theta, err, iters, status, nullptr, nullptr);
  });
}

// Frame sequences on the one-wavefront route: the batch is num_frames x S instances, frame-major, and a wave owns a sequence --
// frame f of sequence s is mmx_solve's MMX_ROUTE_WAVE solve of instance f S + s, started from the result row of frame f - 1.
// Everything that can refuse is settled before theta or an output is touched; kernels only (zeroAsync is one), as mmx_solve.
int32_t mmx_solve_frames(
    mmx_problem* pb,
    const mmx_gn_options* o,
    int32_t num_frames,
    float* theta_dev,
    double* final_error,
    int32_t* iterations,
    int32_t* status,
    double* error_history,
    float* parameter_history,
    void* stream) {
  MMX_ZONE("mmx_solve_frames (SolverT::solve per frame, warm-started along the sequence)");
  MMX_TRY(checkProblem(pb, true));
  if (o == nullptr || theta_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "options / theta is null");
  }
  const SolveOutputs out{final_error, iterations, status, error_history, parameter_history, nullptr};
  const mmx::SolvePlan plan = mmx::planSolveFrames(solveFacts(pb, out, MMX_PRECISION_F32, true), *o, pb->B, num_frames);
  if (plan.code != MMX_OK) {
    return fail(plan.code, plan.message);
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  return runWave(pb, o, theta_dev, out, num_frames, static_cast<hipStream_t>(stream));
}

int32_t mmx_solve_frames_host(
    mmx_problem* pb,
    const mmx_gn_options* o,
    int32_t num_frames,
    float* theta_host,
    double* final_error_host,
    int32_t* iterations_host,
    int32_t* status_host) {
  MMX_ZONE("mmx_solve_frames_host");
  return solveStaged<float>(pb, theta_host, final_error_host, iterations_host, status_host, [&](float* theta, double* err, int32_t* iters, int32_t* status) {
    return mmx_solve_frames(pb, o, num_frames, theta, err, iters, status, nullptr, nullptr, nullptr);
  });
}

int32_t mmx_solve_f64_host(
    mmx_problem* pb,
    const mmx_gn_options* o,
    double* theta_host,
    double* final_error_host,
    int32_t* iterations_host,
    int32_t* status_host) {
  MMX_ZONE("mmx_solve_f64_host");
  return solveStaged<double>(pb, theta_host, final_error_host, iterations_host, status_host, [&](double* theta, double* err, int32_t* iters, int32_t* status) {
    return mmx_solve_f64(pb, o, theta, err, iters, status, nullptr, nullptr);
  });
}

int32_t mmx_eval_gradient(mmx_problem* pb, const float* theta_dev, float* grad_dev, double* err_dev, void* stream) {
  MMX_ZONE("mmx_eval_gradient (getGradient without a Jacobian)");
  MMX_TRY(checkProblem(pb, true));
  if (theta_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta is null");
  }
  if (grad_dev == nullptr && err_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_eval_gradient: grad and err are both null (ask for at least one output)");
  }
  // the scope decision is host code of its own (mmx_solve_plan.cpp): a refusal comes before any output is touched
  mmx::SolveFacts facts; // (the facts gradientRefusal reads; the solves' budgets stay at their defaults)
  facts.numBlocks = pb->dev.numBlocks, facts.G = pb->dev.G, facts.NE = pb->dev.NE;
  facts.instanceParents = pb->dev.instPosParent != nullptr || pb->dev.instOriParent != nullptr;
  facts.U = pb->U, facts.n = pb->fdev.n;
  facts.gradientLdsBytes = mmx::gradientLdsBytes(pb->rig->J, pb->rig->P, pb->U);
  if (const char* why = mmx::gradientRefusal(facts)) {
    return fail(MMX_ERR_UNSUPPORTED, why);
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  const SolveView sv = solveView(pb);
  MMX_HIP(mmx::launchEvalGradient(sv.rig, sv.pb, sv.fd, theta_dev, grad_dev, err_dev, static_cast<hipStream_t>(stream)));
  return MMX_OK;
}

int32_t mmx_eval_gradient_host(mmx_problem* pb, const float* theta_host, float* grad_host, double* err_host) {
  MMX_ZONE("mmx_eval_gradient_host");
  MMX_TRY(checkProblem(pb, true));
  if (theta_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta is null");
  }
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P);
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(pb->sTheta.ensure(B * P * sizeof(float)));
  MMX_HIP(pb->sJtr.ensure(B * P * sizeof(float)));
  MMX_HIP(pb->sErr.ensure(B * sizeof(double)));
  MMX_HIP(hipMemcpy(pb->sTheta.p, theta_host, B * P * sizeof(float), hipMemcpyHostToDevice));
  MMX_TRY(mmx_eval_gradient(pb, pb->sTheta.as<float>(), grad_host != nullptr ? pb->sJtr.as<float>() : nullptr, err_host != nullptr ? pb->sErr.as<double>() : nullptr, nullptr));
  MMX_HIP(hipDeviceSynchronize());
  if (grad_host) {
    MMX_HIP(hipMemcpy(grad_host, pb->sJtr.p, B * P * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (err_host) {
    MMX_HIP(hipMemcpy(err_host, pb->sErr.p, B * sizeof(double), hipMemcpyDeviceToHost));
  }
  return MMX_OK;
}

int32_t mmx_eval_skeleton_state_host(mmx_problem* pb, const float* theta_host, float* state_host) {
  MMX_ZONE("mmx_eval_skeleton_state_host");
  MMX_TRY(checkProblem(pb, false));
  if (theta_host == nullptr || state_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta / state is null");
  }
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P), J = size_t(pb->rig->J);
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(pb->sTheta.ensure(B * P * sizeof(float)));
  MMX_HIP(pb->sRes.ensure(B * J * 8 * sizeof(float)));
  MMX_HIP(hipMemcpy(pb->sTheta.p, theta_host, B * P * sizeof(float), hipMemcpyHostToDevice));
  MMX_TRY(mmx_eval_skeleton_state(pb, pb->sTheta.as<float>(), pb->sRes.as<float>(), nullptr));
  MMX_HIP(hipDeviceSynchronize());
  MMX_HIP(hipMemcpy(state_host, pb->sRes.p, B * J * 8 * sizeof(float), hipMemcpyDeviceToHost));
  return MMX_OK;
}

namespace {
// The rig's tables of the backward pass, on the device: built and uploaded by the first call (the warm-up), kept afterwards
int32_t ensureStateBackwardTables(mmx_rig* rig) {
  static_assert(sizeof(mmx::ColumnSource) == sizeof(mmx::ColumnSourceDev), "ColumnSource layouts must match");
  std::lock_guard<std::mutex> lock(rig->sbMutex);
  if (rig->sbReady) {
    return MMX_OK;
  }
  const mmx::StateBackwardTables t = mmx::buildStateBackwardTables(rig->topo);
  MMX_HIP(upload(rig->dSbSubSize, t.subSize));
  MMX_HIP(upload(rig->dSbLoadedPos, t.loadedPos));
  MMX_HIP(upload(rig->dSbJointPos, t.jointPos));
  MMX_HIP(upload(rig->dSbColStart, t.colStart));
  MMX_HIP(upload(rig->dSbColSources, t.colSources));
  mmx::StateBackwardDev& d = rig->sbDev;
  d.subSize = rig->dSbSubSize.as<int32_t>();
  d.loadedPos = rig->dSbLoadedPos.as<int32_t>();
  d.jointPos = rig->dSbJointPos.as<int32_t>();
  d.colStart = rig->dSbColStart.as<int32_t>();
  d.colSources = rig->dSbColSources.as<mmx::ColumnSourceDev>();
  rig->sbReady = true;
  return MMX_OK;
}
} // namespace

int32_t mmx_eval_skeleton_state_backward(mmx_problem* pb, const float* theta_dev, const float* state_grad_dev, float* theta_grad_dev, void* stream) {
  MMX_ZONE("mmx_eval_skeleton_state_backward (skeleton state VJP)");
  MMX_TRY(checkProblem(pb, false));
  if (theta_dev == nullptr || state_grad_dev == nullptr || theta_grad_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_eval_skeleton_state_backward: theta / state_grad / theta_grad is null");
  }
  // the scope rule is host code of its own (mmx_solve_plan.cpp): a refusal comes before any output is touched
  if (const char* why = mmx::stateBackwardRefusal(mmx::stateBackwardLdsBytes(pb->rig->J, pb->rig->P))) {
    return fail(MMX_ERR_UNSUPPORTED, why);
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_TRY(ensureStateBackwardTables(pb->rig));
  MMX_HIP(mmx::launchStateBackward(pb->rigDev, pb->rig->sbDev, pb->B, theta_dev, state_grad_dev, theta_grad_dev, static_cast<hipStream_t>(stream)));
  return MMX_OK;
}

int32_t mmx_eval_skeleton_state_backward_host(mmx_problem* pb, const float* theta_host, const float* state_grad_host, float* theta_grad_host) {
  MMX_ZONE("mmx_eval_skeleton_state_backward_host");
  MMX_TRY(checkProblem(pb, false));
  if (theta_host == nullptr || state_grad_host == nullptr || theta_grad_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_eval_skeleton_state_backward_host: theta / state_grad / theta_grad is null");
  }
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P), J = size_t(pb->rig->J);
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(pb->sTheta.ensure(B * P * sizeof(float)));
  MMX_HIP(pb->sRes.ensure(B * J * 8 * sizeof(float)));
  MMX_HIP(pb->sJtr.ensure(B * P * sizeof(float)));
  MMX_HIP(hipMemcpy(pb->sTheta.p, theta_host, B * P * sizeof(float), hipMemcpyHostToDevice));
  MMX_HIP(hipMemcpy(pb->sRes.p, state_grad_host, B * J * 8 * sizeof(float), hipMemcpyHostToDevice));
  MMX_TRY(mmx_eval_skeleton_state_backward(pb, pb->sTheta.as<float>(), pb->sRes.as<float>(), pb->sJtr.as<float>(), nullptr));
  MMX_HIP(hipDeviceSynchronize());
  MMX_HIP(hipMemcpy(theta_grad_host, pb->sJtr.p, B * P * sizeof(float), hipMemcpyDeviceToHost));
  return MMX_OK;
}

int32_t mmx_eval_jacobian_host(
    mmx_problem* pb,
    const float* theta_host,
    float* jac_host,
    float* res_host,
    double* err_host,
    int32_t layout) {
  MMX_ZONE("mmx_eval_jacobian_host");
  MMX_TRY(checkProblem(pb, true));
  if (theta_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "theta is null");
  }
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P), M = size_t(pb->M);
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(pb->sTheta.ensure(B * P * sizeof(float)));
  MMX_HIP(pb->sJac.ensure(B * M * P * sizeof(float)));
  MMX_HIP(pb->sRes.ensure(B * std::max<size_t>(M, 1) * sizeof(float)));
  MMX_HIP(pb->sErr.ensure(B * sizeof(double)));
  MMX_HIP(hipMemcpy(pb->sTheta.p, theta_host, B * P * sizeof(float), hipMemcpyHostToDevice));
  MMX_TRY(mmx_eval_jacobian(pb, pb->sTheta.as<float>(), pb->sJac.as<float>(), pb->sRes.as<float>(), pb->sErr.as<double>(), layout, nullptr));
  MMX_HIP(hipDeviceSynchronize());
  if (jac_host) {
    MMX_HIP(hipMemcpy(jac_host, pb->sJac.p, B * M * P * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (res_host) {
    MMX_HIP(hipMemcpy(res_host, pb->sRes.p, B * M * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (err_host) {
    MMX_HIP(hipMemcpy(err_host, pb->sErr.p, B * sizeof(double), hipMemcpyDeviceToHost));
  }
  return MMX_OK;
}

// ---- linear-blend skinning (mmx_skinning.hip; bookkeeping: mmx_skin_tables.cpp)
int32_t mmx_host_skin_tables(
    int32_t num_joints, const mmx_skin_desc* desc, int32_t* joint_start, int32_t* entry_vertex, int32_t* entry_slot, int32_t* num_entries) {
  std::string err;
  const int32_t rc = mmx::validateSkinDesc(num_joints, desc, false, err);
  if (rc != MMX_OK) {
    return fail(rc, "mmx_host_skin_tables: " + err);
  }
  const mmx::SkinTables t = mmx::buildSkinTables(num_joints, desc);
  if (joint_start) {
    std::memcpy(joint_start, t.jointStart.data(), sizeof(int32_t) * t.jointStart.size());
  }
  if (entry_vertex && !t.entryVertex.empty()) {
    std::memcpy(entry_vertex, t.entryVertex.data(), sizeof(int32_t) * t.entryVertex.size());
  }
  if (entry_slot && !t.entrySlot.empty()) {
    std::memcpy(entry_slot, t.entrySlot.data(), sizeof(int32_t) * t.entrySlot.size());
  }
  if (num_entries) {
    *num_entries = int32_t(t.entryVertex.size());
  }
  return MMX_OK;
}

int32_t mmx_skin_create(mmx_rig* rig, const mmx_skin_desc* desc, mmx_skin** out) {
  MMX_ZONE("mmx_skin_create");
  if (out == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_create: out is null");
  }
  *out = nullptr;
  if (rig == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_create: rig handle is null");
  }
  std::string err;
  const int32_t rc = mmx::validateSkinDesc(rig->J, desc, true, err);
  if (rc != MMX_OK) {
    return fail(rc, "mmx_skin_create: " + err);
  }
  if (const char* why = mmx::skinRefusal(rig->J)) {
    return fail(MMX_ERR_UNSUPPORTED, why);
  }
  std::unique_ptr<mmx_skin> sk(new (std::nothrow) mmx_skin());
  if (!sk) {
    return fail(MMX_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  sk->rig = rig;
  const size_t V = size_t(desc->num_vertices), K = size_t(desc->max_influences), J = size_t(rig->J);
  const mmx::SkinTables t = mmx::buildSkinTables(rig->J, desc);
  std::vector<float> ib(J * 12, 0.f);
  for (size_t j = 0; j < J; ++j) {
    if (desc->inverse_bind != nullptr) {
      std::copy(desc->inverse_bind + 12 * j, desc->inverse_bind + 12 * j + 12, ib.begin() + 12 * j);
    } else {
      ib[12 * j] = ib[12 * j + 5] = ib[12 * j + 10] = 1.f;
    }
  }
  MMX_HIP(hipSetDevice(rig->device));
  MMX_HIP(upload(sk->dJoint, std::vector<int32_t>(desc->joint, desc->joint + V * K)));
  MMX_HIP(upload(sk->dWeight, std::vector<float>(desc->weight, desc->weight + V * K)));
  MMX_HIP(upload(sk->dInverseBind, ib));
  MMX_HIP(upload(sk->dRest, std::vector<float>(desc->rest_positions, desc->rest_positions + V * 3)));
  MMX_HIP(upload(sk->dJointStart, t.jointStart));
  MMX_HIP(upload(sk->dEntryVertex, t.entryVertex));
  MMX_HIP(upload(sk->dEntryWeight, t.entryWeight));
  MMX_HIP(upload(sk->dWaveStart, t.waveStart));
  mmx::SkinDev& d = sk->dev;
  d.V = desc->num_vertices, d.K = desc->max_influences, d.J = rig->J, d.numWaves = int32_t(t.waveStart.size()) - 1;
  d.joint = sk->dJoint.as<int32_t>(), d.weight = sk->dWeight.as<float>();
  d.inverseBind = sk->dInverseBind.as<float>(), d.rest = sk->dRest.as<float>();
  d.jointStart = sk->dJointStart.as<int32_t>(), d.entryVertex = sk->dEntryVertex.as<int32_t>();
  d.entryWeight = sk->dEntryWeight.as<float>(), d.waveStart = sk->dWaveStart.as<int32_t>();
  *out = sk.release();
  return MMX_OK;
}

void mmx_skin_destroy(mmx_skin* skin) {
  if (skin != nullptr) {
    if (skin->rig != nullptr) {
      (void)hipSetDevice(skin->rig->device);
    }
    delete skin;
  }
}

int32_t mmx_skin_num_vertices(const mmx_skin* skin) {
  return skin ? skin->dev.V : 0;
}

int32_t mmx_skin_points(mmx_skin* skin, int32_t batch, const float* state_dev, const float* rest_dev, float* out_dev, void* stream) {
  MMX_ZONE("mmx_skin_points (linear-blend skinning)");
  if (skin == nullptr || state_dev == nullptr || out_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points: skin / state / out is null");
  }
  if (batch < 1) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points: batch must be >= 1");
  }
  MMX_HIP(hipSetDevice(skin->rig->device));
  MMX_HIP(mmx::launchSkinPoints(skin->dev, batch, state_dev, rest_dev, out_dev, static_cast<hipStream_t>(stream)));
  return MMX_OK;
}

int32_t mmx_skin_points_backward(
    mmx_skin* skin,
    int32_t batch,
    const float* state_dev,
    const float* rest_dev,
    const float* out_grad_dev,
    float* state_grad_dev,
    float* rest_grad_dev,
    void* stream) {
  MMX_ZONE("mmx_skin_points_backward (linear-blend skinning VJP)");
  if (skin == nullptr || state_dev == nullptr || out_grad_dev == nullptr || state_grad_dev == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points_backward: skin / state / out_grad / state_grad is null");
  }
  if (batch < 1) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points_backward: batch must be >= 1");
  }
  MMX_HIP(hipSetDevice(skin->rig->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  MMX_HIP(mmx::launchSkinPointsBackward(skin->dev, batch, state_dev, rest_dev, out_grad_dev, state_grad_dev, s));
  if (rest_grad_dev != nullptr) {
    MMX_HIP(mmx::launchSkinRestGrad(skin->dev, batch, state_dev, out_grad_dev, rest_grad_dev, s));
  }
  return MMX_OK;
}

int32_t mmx_skin_points_host(mmx_skin* skin, int32_t batch, const float* state_host, const float* rest_host, float* out_host) {
  MMX_ZONE("mmx_skin_points_host");
  if (skin == nullptr || state_host == nullptr || out_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points_host: skin / state / out is null");
  }
  if (batch < 1) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points_host: batch must be >= 1");
  }
  const size_t nState = size_t(batch) * size_t(skin->dev.J) * 8 * sizeof(float), nVert = size_t(batch) * size_t(skin->dev.V) * 3 * sizeof(float);
  MMX_HIP(hipSetDevice(skin->rig->device));
  MMX_HIP(skin->sState.ensure(nState));
  MMX_HIP(skin->sOut.ensure(nVert));
  MMX_HIP(hipMemcpy(skin->sState.p, state_host, nState, hipMemcpyHostToDevice));
  if (rest_host != nullptr) {
    MMX_HIP(skin->sRest.ensure(nVert));
    MMX_HIP(hipMemcpy(skin->sRest.p, rest_host, nVert, hipMemcpyHostToDevice));
  }
  MMX_TRY(mmx_skin_points(skin, batch, skin->sState.as<float>(), rest_host ? skin->sRest.as<float>() : nullptr, skin->sOut.as<float>(), nullptr));
  MMX_HIP(hipDeviceSynchronize());
  MMX_HIP(hipMemcpy(out_host, skin->sOut.p, nVert, hipMemcpyDeviceToHost));
  return MMX_OK;
}

int32_t mmx_skin_points_backward_host(
    mmx_skin* skin,
    int32_t batch,
    const float* state_host,
    const float* rest_host,
    const float* out_grad_host,
    float* state_grad_host,
    float* rest_grad_host) {
  MMX_ZONE("mmx_skin_points_backward_host");
  if (skin == nullptr || state_host == nullptr || out_grad_host == nullptr || state_grad_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points_backward_host: skin / state / out_grad / state_grad is null");
  }
  if (batch < 1) {
    return fail(MMX_ERR_INVALID_ARGUMENT, "mmx_skin_points_backward_host: batch must be >= 1");
  }
  const size_t nState = size_t(batch) * size_t(skin->dev.J) * 8 * sizeof(float), nVert = size_t(batch) * size_t(skin->dev.V) * 3 * sizeof(float);
  MMX_HIP(hipSetDevice(skin->rig->device));
  MMX_HIP(skin->sState.ensure(nState));
  MMX_HIP(skin->sOut.ensure(nVert));
  MMX_HIP(skin->sStateGrad.ensure(nState));
  MMX_HIP(hipMemcpy(skin->sState.p, state_host, nState, hipMemcpyHostToDevice));
  MMX_HIP(hipMemcpy(skin->sOut.p, out_grad_host, nVert, hipMemcpyHostToDevice));
  if (rest_host != nullptr) {
    MMX_HIP(skin->sRest.ensure(nVert));
    MMX_HIP(hipMemcpy(skin->sRest.p, rest_host, nVert, hipMemcpyHostToDevice));
  }
  if (rest_grad_host != nullptr) {
    MMX_HIP(skin->sRestGrad.ensure(nVert));
  }
  MMX_TRY(mmx_skin_points_backward(
      skin, batch, skin->sState.as<float>(), rest_host ? skin->sRest.as<float>() : nullptr, skin->sOut.as<float>(), skin->sStateGrad.as<float>(),
      rest_grad_host ? skin->sRestGrad.as<float>() : nullptr, nullptr));
  MMX_HIP(hipDeviceSynchronize());
  MMX_HIP(hipMemcpy(state_grad_host, skin->sStateGrad.p, nState, hipMemcpyDeviceToHost));
  if (rest_grad_host != nullptr) {
    MMX_HIP(hipMemcpy(rest_grad_host, skin->sRestGrad.p, nVert, hipMemcpyDeviceToHost));
  }
  return MMX_OK;
}

// ---- Gauss-Newton terms of vertex constraints on a skin (mmx_skin_normal_equations.hip; intake: mmx_vertex_constraints.cpp)
} // extern "C"

// the intake both device entries share: the refusals of mmx_skin_normal_equations in their order (pure host), then the
// kernel's descriptors.  `ldsBytes` (optional) receives the call's LDS size.
static int32_t skinNormalEquationsIntake(
    const char* name,
    mmx_problem* pb,
    mmx_skin* skin,
    const mmx_vertex_constraints* c,
    bool haveTheta,
    bool haveOutput,
    mmx::SkinNeColumnsDev* cols,
    mmx::VertexConstraintsDev* vc,
    size_t* ldsBytes) {
  MMX_TRY(checkProblem(pb, false));
  if (skin == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, std::string(name) + ": skin handle is null");
  }
  const mmx::ProblemDev& d = pb->dev;
  const int32_t nsrc = int32_t(pb->tables.colSources.size());
  mmx::VertexConstraintsFacts f;
  f.sameRig = skin->rig == pb->rig;
  f.haveTheta = haveTheta;
  f.haveOutput = haveOutput;
  f.skinVertices = skin->dev.V;
  f.solved = d.n;
  if (c != nullptr && (c->corners == 1 || c->corners == 3) && d.n >= 1 && d.n <= mmx::kSkinNeMaxSolved) {
    f.ldsBytes = mmx::skinNormalEquationsLdsBytes(pb->rig->J, pb->rig->P, d.n, nsrc, c->corners, skin->dev.K);
  }
  std::string err;
  const int32_t rc = mmx::checkVertexConstraints(c, f, err);
  if (rc != MMX_OK) {
    return fail(rc, std::string(name) + ": " + err);
  }
  cols->n = d.n, cols->nsrc = nsrc;
  cols->enabledList = d.enabledList, cols->colStart = d.colStart, cols->colSources = d.colSources, cols->jointTin = d.jointTin;
  vc->type = c->type, vc->C = c->count, vc->S = c->corners, vc->fw = c->function_weight;
  vc->vertex = c->vertex, vc->bary = c->corners == 3 ? c->barycentric : nullptr, vc->target = c->target;
  vc->normal = c->type == MMX_VC_PLANE ? c->normal : nullptr, vc->weight = c->weight, vc->rest = c->rest;
  if (ldsBytes != nullptr) {
    *ldsBytes = f.ldsBytes;
  }
  return MMX_OK;
}

// parts = 0: the plan, fed with the device's compute units and the workgroups of this call's LDS size a compute unit holds
static int32_t skinNormalEquationsAutoParts(const char* name, mmx_problem* pb, int32_t type, int32_t count, size_t ldsBytes, int32_t* parts) {
  int cus = 0;
  MMX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, pb->rig->device));
  const int32_t perCu = 2 * ldsBytes <= size_t(160) * 1024 ? 2 : 1; // (registers bind at two: DESIGN.md)
  if (!mmx::skinNePlan(pb->B, type, count, cus, perCu, parts)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, std::string(name) + ": the plan refuses the batch, count, type or compute-unit count");
  }
  return MMX_OK;
}

extern "C" {

int32_t mmx_skin_normal_equations(
    mmx_problem* pb,
    mmx_skin* skin,
    const mmx_vertex_constraints* c,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    double* err_dev,
    void* stream) {
  MMX_ZONE("mmx_skin_normal_equations (vertex constraints: JtJ, JtR, error)");
  mmx::SkinNeColumnsDev cols{};
  mmx::VertexConstraintsDev vc{};
  MMX_TRY(skinNormalEquationsIntake(
      "mmx_skin_normal_equations", pb, skin, c, theta_dev != nullptr, jtj_dev != nullptr || jtr_dev != nullptr || err_dev != nullptr, &cols, &vc,
      nullptr));
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(mmx::launchSkinNormalEquations(pb->rigDev, cols, skin->dev, vc, pb->B, theta_dev, jtj_dev, jtr_dev, err_dev, static_cast<hipStream_t>(stream)));
  return MMX_OK;
}

int32_t mmx_skin_normal_equations_split(
    mmx_problem* pb,
    mmx_skin* skin,
    const mmx_vertex_constraints* c,
    const float* theta_dev,
    float* jtj_dev,
    float* jtr_dev,
    double* err_dev,
    int32_t parts,
    void* workspace_dev,
    int64_t workspace_bytes,
    void* stream) {
  MMX_ZONE("mmx_skin_normal_equations_split (vertex constraints over several workgroups per instance)");
  static const char* kName = "mmx_skin_normal_equations_split";
  mmx::SkinNeColumnsDev cols{};
  mmx::VertexConstraintsDev vc{};
  size_t ldsBytes = 0;
  MMX_TRY(skinNormalEquationsIntake(
      kName, pb, skin, c, theta_dev != nullptr, jtj_dev != nullptr || jtr_dev != nullptr || err_dev != nullptr, &cols, &vc, &ldsBytes));
  std::string err;
  int32_t rc = mmx::checkSkinNeParts(parts, err);
  if (rc != MMX_OK) {
    return fail(rc, std::string(kName) + ": " + err);
  }
  mmx::SkinNeSplitFacts f;
  f.batch = pb->B, f.solved = cols.n, f.type = vc.type, f.count = vc.C;
  f.requested = parts, f.parts = parts;
  if (parts == 0) {
    MMX_TRY(skinNormalEquationsAutoParts(kName, pb, vc.type, vc.C, ldsBytes, &f.parts));
  }
  f.haveWorkspace = workspace_dev != nullptr;
  f.workspaceAddress = reinterpret_cast<uintptr_t>(workspace_dev);
  f.workspaceBytes = workspace_bytes;
  rc = mmx::checkSkinNeSplit(f, err);
  if (rc != MMX_OK) {
    return fail(rc, std::string(kName) + ": " + err);
  }
  MMX_HIP(hipSetDevice(pb->rig->device));
  MMX_HIP(mmx::launchSkinNormalEquationsSplit(
      pb->rigDev, cols, skin->dev, vc, pb->B, theta_dev, jtj_dev, jtr_dev, err_dev, f.parts, workspace_dev, static_cast<hipStream_t>(stream)));
  return MMX_OK;
}

int64_t mmx_skin_normal_equations_workspace_bytes(int32_t batch, int32_t num_enabled, int32_t parts) {
  return mmx::skinNeWorkspaceBytes(batch, num_enabled, parts);
}

int32_t mmx_skin_normal_equations_plan(
    int32_t batch, int32_t type, int32_t count, int32_t compute_units, int32_t workgroups_per_cu, int32_t* parts_out) {
  int32_t parts = 0;
  if (!mmx::skinNePlan(batch, type, count, compute_units, workgroups_per_cu, &parts)) {
    return fail(
        MMX_ERR_INVALID_ARGUMENT,
        "mmx_skin_normal_equations_plan: batch, count, compute_units and workgroups_per_cu must be >= 1 and type MMX_VC_POSITION or MMX_VC_PLANE");
  }
  if (parts_out != nullptr) {
    *parts_out = parts;
  }
  return MMX_OK;
}

int32_t mmx_skin_normal_equations_part_range(
    int32_t tiles, int32_t parts, int32_t part, int32_t* begin_out, int32_t* end_out, int32_t* effective_parts_out) {
  if (tiles < 1 || parts < 1 || parts > mmx::kSkinNeMaxParts || part < 0 || part >= mmx::skinNeEffectiveParts(parts, tiles)) {
    return fail(
        MMX_ERR_INVALID_ARGUMENT,
        "mmx_skin_normal_equations_part_range: tiles must be >= 1, parts in 1..MMX_SKIN_NE_MAX_PARTS and part in [0, min(parts, tiles))");
  }
  const int32_t pe = mmx::skinNeEffectiveParts(parts, tiles);
  if (begin_out != nullptr) {
    *begin_out = mmx::skinNePartBegin(part, tiles, pe);
  }
  if (end_out != nullptr) {
    *end_out = mmx::skinNePartBegin(part + 1, tiles, pe);
  }
  if (effective_parts_out != nullptr) {
    *effective_parts_out = pe;
  }
  return MMX_OK;
}

int32_t mmx_skin_normal_equations_auto_parts(mmx_problem* pb, mmx_skin* skin, const mmx_vertex_constraints* c, int32_t* parts_out) {
  static const char* kName = "mmx_skin_normal_equations_auto_parts";
  MMX_TRY(checkProblem(pb, false));
  if (skin == nullptr || c == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, std::string(kName) + ": skin / constraints is null");
  }
  if (skin->rig != pb->rig) {
    return fail(MMX_ERR_INVALID_ARGUMENT, std::string(kName) + ": the skin was created on another rig than the problem's");
  }
  if ((c->type != MMX_VC_POSITION && c->type != MMX_VC_PLANE) || c->count < 1 || (c->corners != 1 && c->corners != 3)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, std::string(kName) + ": unknown type, count < 1 or corners outside {1, 3}");
  }
  const int32_t n = pb->dev.n;
  if (n < 1 || n > mmx::kSkinNeMaxSolved) {
    return fail(MMX_ERR_UNSUPPORTED, std::string(kName) + ": the enabled parameters are outside 1..MMX_SKIN_NE_MAX_SOLVED (128)");
  }
  const size_t lds = mmx::skinNormalEquationsLdsBytes(pb->rig->J, pb->rig->P, n, int32_t(pb->tables.colSources.size()), c->corners, skin->dev.K);
  if (lds > mmx::kVertexConstraintsLdsBudget) {
    return fail(MMX_ERR_UNSUPPORTED, std::string(kName) + ": the tables do not fit the kernel's LDS budget (160 KB)");
  }
  int32_t parts = 0;
  MMX_TRY(skinNormalEquationsAutoParts(kName, pb, c->type, c->count, lds, &parts));
  if (parts_out != nullptr) {
    *parts_out = parts;
  }
  return MMX_OK;
}

} // extern "C"

// the two _host forms: stage the descriptor's arrays and theta, run the device entry (split false: the unsplit one; else the
// split one with a workspace allocated and freed here -- the device entry refuses a `parts` out of range, after the unsplit
// refusals as documented), copy the outputs back
static int32_t skinNormalEquationsHost(
    const char* name,
    mmx_problem* pb,
    mmx_skin* skin,
    const mmx_vertex_constraints* c,
    const float* theta_host,
    float* jtj_host,
    float* jtr_host,
    double* err_host,
    bool split,
    int32_t parts) {
  MMX_TRY(checkProblem(pb, false));
  if (skin == nullptr || c == nullptr || theta_host == nullptr) {
    return fail(MMX_ERR_INVALID_ARGUMENT, std::string(name) + ": skin / constraints / theta is null");
  }
  if (c->count < 1 || (c->corners != 1 && c->corners != 3)) {
    return fail(MMX_ERR_INVALID_ARGUMENT, std::string(name) + ": count must be >= 1 and corners 1 or 3");
  }
  const size_t B = size_t(pb->B), P = size_t(pb->rig->P), n = size_t(pb->dev.n), C = size_t(c->count), S = size_t(c->corners);
  const size_t V = size_t(skin->dev.V);
  MMX_HIP(hipSetDevice(pb->rig->device));
  mmx_vertex_constraints dv = *c;
  auto stage = [&](DevBuf& buf, const void* src, size_t bytes, const void** out) -> hipError_t {
    *out = nullptr;
    if (src == nullptr) {
      return hipSuccess;
    }
    hipError_t e = buf.ensure(bytes);
    if (e != hipSuccess) {
      return e;
    }
    *out = buf.p;
    return hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice);
  };
  const void* q = nullptr;
  MMX_HIP(stage(skin->sVcVertex, c->vertex, B * C * S * sizeof(int32_t), &q));
  dv.vertex = static_cast<const int32_t*>(q);
  MMX_HIP(stage(skin->sVcBary, c->barycentric, B * C * S * sizeof(float), &q));
  dv.barycentric = static_cast<const float*>(q);
  MMX_HIP(stage(skin->sVcTarget, c->target, B * C * 3 * sizeof(float), &q));
  dv.target = static_cast<const float*>(q);
  MMX_HIP(stage(skin->sVcNormal, c->normal, B * C * 3 * sizeof(float), &q));
  dv.normal = static_cast<const float*>(q);
  MMX_HIP(stage(skin->sVcWeight, c->weight, B * C * sizeof(float), &q));
  dv.weight = static_cast<const float*>(q);
  MMX_HIP(stage(skin->sRest, c->rest, B * V * 3 * sizeof(float), &q));
  dv.rest = static_cast<const float*>(q);
  MMX_HIP(stage(skin->sVcTheta, theta_host, B * P * sizeof(float), &q));
  if (jtj_host != nullptr) {
    MMX_HIP(skin->sVcJtj.ensure(B * n * n * sizeof(float)));
  }
  if (jtr_host != nullptr) {
    MMX_HIP(skin->sVcJtr.ensure(B * n * sizeof(float)));
  }
  if (err_host != nullptr) {
    MMX_HIP(skin->sVcErr.ensure(B * sizeof(double)));
  }
  float* jtjDev = jtj_host ? skin->sVcJtj.as<float>() : nullptr;
  float* jtrDev = jtr_host ? skin->sVcJtr.as<float>() : nullptr;
  double* errDev = err_host ? skin->sVcErr.as<double>() : nullptr;
  if (!split) {
    MMX_TRY(mmx_skin_normal_equations(pb, skin, &dv, skin->sVcTheta.as<float>(), jtjDev, jtrDev, errDev, nullptr));
  } else {
    int32_t resolved = parts;
    if (parts == 0) {
      MMX_TRY(mmx_skin_normal_equations_auto_parts(pb, skin, &dv, &resolved));
    }
    const int64_t bytes = mmx::skinNeWorkspaceBytes(pb->B, pb->dev.n, resolved); // (-1 for a problem or parts the call refuses anyway)
    void* ws = nullptr;
    if (bytes > 0) {
      MMX_HIP(hipMalloc(&ws, size_t(bytes)));
    }
    const int32_t rc = mmx_skin_normal_equations_split(
        pb, skin, &dv, skin->sVcTheta.as<float>(), jtjDev, jtrDev, errDev, parts == 0 ? resolved : parts, ws, bytes > 0 ? bytes : 0, nullptr);
    const hipError_t sync = rc == MMX_OK ? hipDeviceSynchronize() : hipSuccess;
    if (ws != nullptr) {
      (void)hipFree(ws);
    }
    MMX_TRY(rc);
    MMX_HIP(sync);
  }
  MMX_HIP(hipDeviceSynchronize());
  if (jtj_host != nullptr) {
    MMX_HIP(hipMemcpy(jtj_host, skin->sVcJtj.p, B * n * n * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (jtr_host != nullptr) {
    MMX_HIP(hipMemcpy(jtr_host, skin->sVcJtr.p, B * n * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (err_host != nullptr) {
    MMX_HIP(hipMemcpy(err_host, skin->sVcErr.p, B * sizeof(double), hipMemcpyDeviceToHost));
  }
  return MMX_OK;
}

extern "C" {

int32_t mmx_skin_normal_equations_host(
    mmx_problem* pb,
    mmx_skin* skin,
    const mmx_vertex_constraints* c,
    const float* theta_host,
    float* jtj_host,
    float* jtr_host,
    double* err_host) {
  MMX_ZONE("mmx_skin_normal_equations_host");
  return skinNormalEquationsHost("mmx_skin_normal_equations_host", pb, skin, c, theta_host, jtj_host, jtr_host, err_host, false, 1);
}

int32_t mmx_skin_normal_equations_split_host(
    mmx_problem* pb,
    mmx_skin* skin,
    const mmx_vertex_constraints* c,
    const float* theta_host,
    float* jtj_host,
    float* jtr_host,
    double* err_host,
    int32_t parts) {
  MMX_ZONE("mmx_skin_normal_equations_split_host");
  return skinNormalEquationsHost("mmx_skin_normal_equations_split_host", pb, skin, c, theta_host, jtj_host, jtr_host, err_host, true, parts);
}

} // extern "C"
