// mmx_host_tables.hpp -- host-side integer bookkeeping of the batched-IK path (no HIP here, so it
// is unit-testable bit-exactly without a GPU).  Everything in this file is index arithmetic:
// tree levels and DFS intervals of the Skeleton, the enabled-parameter list of
// GaussNewtonSolverT::updateEnabledParameters (momentum/solver/gauss_newton_solver.cpp:57-66),
// ParameterTransformT::computeActiveJointParams (momentum/character/parameter_transform.cpp:97-107)
// and a column-wise (CSC) view of the enabled part of the parameter transform, which is what lets
// the kernels GATHER a Jacobian column instead of scattering like the reference's ancestor walk
// (momentum/character_solver/joint_error_function-inl.h:228-294).  The second half of the file builds every table a problem
// uploads (slots, term records, limit tables, tile structure, the live-joint view): tests/cpp/test_problem_tables.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mmx.h"

namespace mmx {

// One source term of a Jacobian column p: joint-parameter row (joint, dof) of the parameter
// transform with weight w = transform(7*joint+dof, p).  tin/tout = DFS interval of `joint`:
// the term contributes to a constraint on joint j iff tin <= tin[j] < tout (joint is j or one of
// its ancestors -- exactly the set the reference's while(jntIndex != kInvalidIndex) loop visits).
struct ColumnSource {
  int32_t joint;
  int32_t dof; // 0..2 translation, 3..5 rotation, 6 scale
  int32_t tin;
  int32_t tout;
  int32_t parent; // parent joint of `joint` (-1 for a root): translationAxis = parent.toLinear()
  float weight;
};

// One record of the J-assembly kernel's column program: a Jacobian column with exactly ONE
// source that is a ROTATION dof -- the overwhelmingly common case -- listed grouped by joint so
// that the kernel computes the ancestor test and v - t_joint once per joint.
// 32 bytes = one s_load_dwordx8.
struct JacRec {
  int32_t joint, dof, col, tin, tout, parent;
  float weight;
  int32_t valid; // unused (padding records are copies of the last real record)
};

struct HostTables {
  int32_t J = 0, P = 0;
  // --- skeleton topology
  std::vector<int32_t> level; // [J] depth, root = 0
  std::vector<int32_t> levelOrder; // [J] joints sorted by (level, index)
  std::vector<int32_t> levelStart; // [numLevels+1] offsets into levelOrder
  std::vector<int32_t> tin, tout; // [J] DFS pre-order interval
  // --- enabled-parameter dependent
  std::vector<uint8_t> enabled; // [P]
  std::vector<uint8_t> activeJointParams; // [7J]
  std::vector<int32_t> enabledList; // [n] ascending
  std::vector<int32_t> fullToSubset; // [P] index into enabledList or -1
  // the enabled parameters in ELIMINATION order (a permutation of enabledList): the order in which the solvers number
  // the columns of their normal equations.  Two columns of J overlap only when a joint of the one is an ancestor of a
  // joint of the other, so with every subtree's parameters ahead of those of the joints above it (a post-order of the
  // skeleton, small subtrees first) the Cholesky factor of J^T J fills in next to nothing outside that ancestor pattern
  // -- the blocked solvers skip the 16 x 16 tiles that stay zero (eliminationTileMasks).  The reference's dense QR has
  // no such order; the step it computes does not depend on one.
  std::vector<int32_t> eliminationList;
  std::vector<int32_t> colStart; // [P+1] offsets into colSources (disabled columns are empty)
  std::vector<ColumnSource> colSources;
  int32_t maxColSources = 0;
  // column program of the J-assembly kernel
  std::vector<JacRec> jacRecs; // single-source rotation columns, grouped by joint, padded to a multiple of 4
  std::vector<int32_t> multiCols; // all other non-empty columns (generic gather path)
  std::vector<int32_t> zeroCols; // columns without sources (disabled parameters): written as zeros
};

// Tables of the fused solve kernel, for one (rig, constraint topology, enabled set):
//  - joints in DFS pre-order, so that the subtree of a joint is a contiguous index range
//  - the constraint vectors ("units", 3 Jacobian rows each) attached to each joint
//  - the SOLVE list: enabled parameters whose Jacobian column is not structurally zero, i.e. that
//    drive at least one joint with a constrained joint in its subtree.  A structurally zero column
//    has H row/col = 0 and g = 0, so the reference's step for it is exactly 0 / (0 + lambda) = 0
//    (gauss_newton_solver.cpp:248-257); dropping it from the dense system changes nothing.
struct FusedTables {
  int32_t U = 0; // units = Kp + 3 Ko
  std::vector<int32_t> dfsJoint; // [J] joint at DFS position k
  std::vector<int32_t> subSize; // [J] subtree size of the joint at DFS position k
  std::vector<int32_t> unitJoint; // [U]
  std::vector<int32_t> posUnitStart; // [J+1] CSR over DFS positions -> units attached to that joint
  std::vector<int32_t> posUnits; // [U]
  std::vector<uint8_t> structNonZero; // [P] the parameter's column of the joint-constraint rows can be non-zero
  std::vector<int32_t> solveList; // [n] parameter index of compacted column s (in HostTables::eliminationList order)
  std::vector<int32_t> srcStart; // [n+1] offsets into srcs per compacted column
  std::vector<ColumnSource> srcs;
  int32_t maxDepth = 0;
};

int32_t buildFusedTables(
    const mmx_rig_desc* d,
    const HostTables& t,
    int32_t Kp,
    const int32_t* posParent,
    int32_t Ko,
    const int32_t* oriParent,
    const uint8_t* forceSolve, // [P] or null: enabled parameters to keep in the solve list although
                               // no joint constraint reaches them (limit / model-parameter rows)
    const std::vector<int32_t>* unionPos, // or null: with per-instance constraint parents, every joint that
    const std::vector<int32_t>* unionOri, // carries a position / an orientation constraint in SOME element
    FusedTables& out,
    std::string& err);

// Tile structure of the Cholesky factor of H = J^T J + (parameter-space rows) for a solve list in elimination order:
// `related(row, col)` (row > col) says whether entry (row, col) of H can be non-zero.  Symbolic factorisation on the
// 16 x 16 tile grid (tile (I, J) of L is non-zero when it is in H or when two tiles (I, k), (J, k), k < J, are).
// rowMask[I]: bit J set = tile (I, J <= I) of L is structurally non-zero; colMask[k]: bit I set = tile (I >= k, k) is.
// n <= 512 (32 blocks).  Integer bookkeeping, unit-tested on the CPU.
struct TileMasks {
  int32_t NB = 0;
  uint32_t rowMask[32] = {};
  uint32_t colMask[32] = {};
  std::vector<int32_t> tiles; // the non-zero tiles, I | J << 8, in tile-index order (I (I + 1) / 2 + J ascending)
  int64_t products = 0; // tile products L(I,j) L(k,j)^T of the masked factorisation (dense: NB (NB^2 - 1) / 6)
  // Level schedule of the factorisation (the resident factor kernel): block column k can be factored once every column j
  // with a tile (k, j) is -- level[k] = 1 + max level[j] --, so the columns of one level are independent (the subtrees of
  // the skeleton's elimination tree: finger chains next to the spine's).  steps: [numSteps, then 4 words per step], a word
  // = k | firstWave << 8 | numWaves << 12 (a column's panel of nt tiles takes ceil((16 nt - 16) / 48) of the workgroup's
  // four waves, at least one; 0xf = the whole workgroup, for panels beyond 208 rows) or -1; the columns of a step are
  // factored side by side.
  std::vector<int32_t> levelSteps;
};
TileMasks eliminationTileMasks(int32_t n, const std::vector<uint8_t>& related /* [n][n], lower triangle used */, bool dense);

// mmx_solve_f64's assembly list (mmx::F64AssemblyList, mmx_kernels.hpp) for chunks of `unitsPerChunk` units: every entry
// (solved column, unit) of J with an applicable source -- the source's joint an ancestor-or-self of the unit's joint (DFS
// interval) and, for translation / scale dofs, a point unit (joint_error_function-inl.h:248-291) -- with the indices of
// those sources in the kernel's packed table (columns in solve-list order, a column's sources in colSources order).
// groups: two words per entry, column | unit-in-chunk << 12 | count << 18 and (count == 1 ? the source : offset into
// extra); chunkStart: [chunks + 1] first group of a chunk, then [chunks] the chunk's mask of 16-column blocks with an entry.
// Units: Kp position constraints (points), then three per orientation constraint.  False when a count does not fit.
struct F64AssemblyListHost {
  std::vector<uint32_t> groups;
  std::vector<int32_t> extra, chunkStart;
};
bool buildF64AssemblyListHost(
    const HostTables& t, const std::vector<int32_t>& solveList, const int32_t* posParent, int32_t Kp, const int32_t* oriParent, int32_t Ko,
    int32_t unitsPerChunk, F64AssemblyListHost& out);

// The joints a problem's solve can depend on: the ancestors-or-self of every joint it references (constraint parents, both
// joints of the further blocks and of ellipsoid limits, the joints of joint-parameter limits).  A joint outside that set has
// no constraint in its subtree: its parameters' columns are structurally zero and no residual reads its state, so the solve
// kernels run over the live joints only, renumbered.  Both maps are MONOTONE (compactOf in joint index, compactPos in DFS
// position), so every sum over joints or positions keeps its order -- the pruned solve reproduces the unpruned one bit for bit.
// Pruning nothing is the identity: with no referenced joint, or with every joint live, all J joints are kept.
struct LiveJoints {
  int32_t numLive = 0; // joints kept (J when nothing is pruned)
  std::vector<uint8_t> live; // [J]
  std::vector<int32_t> compactOf; // [J] index among the live joints, -1 for a dead one
  std::vector<int32_t> fullOf; // [numLive] ascending
  bool identity() const {
    return numLive == int32_t(live.size());
  }
};
void buildLiveJoints(const int32_t* parent, int32_t J, const int32_t* joints, int32_t n, LiveJoints& out);

// Validates the descriptor the way the reference's constructors / MT_CHECKs do
// (skeleton.cpp:16-22 parent-before-child; parameter_transform.cpp:112-121 sizes).
// Returns MMX_OK or an error code with a message in `err`.
int32_t validateRigDesc(const mmx_rig_desc* d, std::string& err);

// Builds all tables.  `enabled` may be null (= all parameters enabled).
int32_t buildHostTables(const mmx_rig_desc* d, const uint8_t* enabled, HostTables& out, std::string& err);

// Tables of mmx_eval_skeleton_state_backward, from the rig alone (no constraint, no enabled mask): the joints in DFS
// pre-order with their subtree sizes, EVERY position as a loaded one (each joint's state is an output and carries a
// cotangent), and per model parameter the sources of ALL its transform entries in row order -- colStart / colSources of
// buildHostTables with every parameter enabled, taken over as they are.  Built once per rig and never by a constraint update.
struct StateBackwardTables {
  std::vector<int32_t> dfsJoint; // [J] joint at DFS position k
  std::vector<int32_t> subSize; // [J] subtree size of the joint at DFS position k
  std::vector<int32_t> loadedPos; // [J] 0 .. J-1
  std::vector<int32_t> jointPos; // [J] DFS position of joint j (= tin)
  std::vector<int32_t> colStart; // [P+1]
  std::vector<ColumnSource> colSources;
};
StateBackwardTables buildStateBackwardTables(const HostTables& allEnabled);

// ---------------------------------------------------------------------------------------------------------------------
// Problem tables.  Everything below is what mmx_capi.hip uploads for a problem (uploadProblemTables, uploadSolveView): the
// upload path gathers a ProblemTopology from its handle, calls these builders and copies the vectors to the device.  One
// function per table family, each callable on its own.  They are internal to the library: the exported interface stays the C ABI.
#pragma GCC visibility push(hidden)

// model parameters that can carry a non-zero Jacobian entry of a limit row
std::vector<int32_t> limitParameters(const mmx_rig_desc* d, const mmx_parameter_limit& lm);

// Tables derived from a rig's host arrays: the two-slot ELL copy of the parameter transform (one 16-byte record per
// joint-parameter row), the packed parent / jump-target table, the records of the non-empty transform rows
// (RigDev::ptRowRec) and the pointer-jumping round count.  mmx_rig_create builds them for the rig, the live-joint view of a
// problem for its joints.
struct RigDerived {
  std::vector<int32_t> ell, jumpParent, rowRec;
  bool ellOk = true;
  int32_t jumpRounds = 0;
};
RigDerived deriveRigTables(
    int32_t J, int32_t P, const std::vector<int32_t>& parent, const std::vector<int32_t>& ptOuter, const std::vector<int32_t>& ptInner,
    const std::vector<float>& ptValue, int32_t numLevels);

// What a problem references, as plain data.
struct ProblemTopology {
  int32_t Kp = 0, Ko = 0;
  std::vector<int32_t> posParent, oriParent; // [Kp], [Ko]
  bool instPos = false, instOri = false; // per-instance constraint parents: unionPos / unionOri apply
  std::vector<int32_t> unionPos, unionOri; // joints that carry a position / orientation constraint in some element
  struct Block {
    int32_t type = 0; // MMX_JC_*
    std::vector<int32_t> parent;
    std::vector<int32_t> parentB; // MMX_JC_JOINT_TO_JOINT_DISTANCE: the second joint of every constraint, else empty
  };
  std::vector<Block> blocks;
  std::vector<mmx_ellipsoid_limit> ellipsoids;
  std::vector<mmx_parameter_limit> limits;
  bool hasModel = false; // the model-parameter block is present
  int32_t U() const {
    return Kp + 3 * Ko;
  }
};

// The joints the problem references (LiveJoints): constraint parents, the joints of the further blocks and of ellipsoid
// limits, the joints of joint-parameter limits.
std::vector<int32_t> referencedJoints(const ProblemTopology& p);

// Float offset of entry (row, col), row >= col, in the tile region of H: 16 x 16 tiles in I (I + 1) / 2 + J order, a tile's
// rows 16 floats apart with their four-float groups swizzled by the row (tileAddr() of the kernels).
inline int32_t tileAddress(int32_t row, int32_t col) {
  const int32_t I = row >> 4, Jc = col >> 4, r = row & 15, c = col & 15;
  return (I * (I + 1) / 2 + Jc) * 256 + r * 16 + ((((c >> 2) ^ (r >> 2)) & 3) << 2) + (c & 3);
}

// The tables indexed by joint: units, the flattened constraints of the further blocks ([G], then [G] second joints: the B
// joint of a pair constraint, -1 for every other type) and the joint words of the ellipsoid records.  `compactOf` renumbers
// the joints (null: as they are) and tin / tout are indexed by the renumbered joint, so the full tables and the live-joint
// view are the same code.
struct JointTables {
  std::vector<int32_t> unitJoint, unitTin; // [max(U, 1)]
  std::vector<int32_t> genJoint, genTin; // [2 G]
  std::vector<int32_t> genBlock; // [G]
  std::vector<int32_t> ellParent, ellEllipsoidParent; // [NE]
  std::vector<int32_t> ellTinParent; // [NE] tin[parent]
  std::vector<int32_t> ellTinStop; // [NE] tin[ellipsoidParent] when that joint is an ancestor-or-self of `parent`, else -1
};
JointTables buildJointTables(const ProblemTopology& p, const int32_t* compactOf, const std::vector<int32_t>& tin, const std::vector<int32_t>& tout);

// What buildFusedTables is fed beside the constraint parents: the parameters a limit or (all of them) the model-parameter
// block touches stay in the solve list; joints that carry a further joint error function or an ellipsoid limit count like
// constrained joints for the structure -- point-like ones (projection, distance and BOTH joints of a pair among them) see
// every dof above them, fixed-axis ones rotations only.
struct StructureLists {
  std::vector<uint8_t> force; // [P]
  std::vector<int32_t> structPos, structOri;
};
StructureLists buildStructureLists(const mmx_rig_desc* d, const ProblemTopology& p);
// ... and buildFusedTables called with them
int32_t buildProblemFusedTables(
    const mmx_rig_desc* d, const HostTables& t, const ProblemTopology& p, const StructureLists& s, FusedTables& out, std::string& err);

// Column program of the J-assembly kernel, specialised to the problem: a column whose sources have no constraint vector
// below them (or that is disabled) is structurally zero -- it moves to the zero list, which the kernel writes BEFORE forward
// kinematics; the rest as in buildHostTables.
struct ColumnProgram {
  std::vector<JacRec> recs; // sorted by (joint, dof), padded to a multiple of 4 with copies of the last record
  std::vector<int32_t> multi, zero;
};
ColumnProgram buildColumnProgram(const HostTables& t, const FusedTables& f);

// Source SLOTS of the fused kernel.  Column c of the compacted system keeps its first source in slot c (the "primary"
// source: with it alone the slot index IS the column index, so the 16 x 16 tiles of H = J^T J come straight out of
// matrix-core products of the per-slot moment contractions); slots n .. slotBase-1 pad the last block (weight 0); the further
// sources of multi-source columns (shared parameters) follow from slot slotBase on, in column order: extras of column c =
// slots slotBase + xStart[c] .. slotBase + xStart[c+1] - 1.  slotBase = 16 * slotBlocks; the caller picks the block count
// (the kernels' instantiations).  The slot count is a multiple of 4.
struct SlotTables {
  int32_t slotBase = 0;
  std::vector<int32_t> loadedPos; // DFS positions that carry a unit, ascending
  std::vector<ColumnSource> slots;
  std::vector<int32_t> xStart; // [slotBase + 1]
  std::vector<int32_t> slotOf; // [srcs] source e of FusedTables::srcs -> its slot
};
SlotTables buildSlotTables(const FusedTables& f, int32_t slotBlocks);

// Structural term records of H for the pairs the matrix-core pass does not cover: entry (row, col), row >= col, receives one
// term per pair (source a of row, source c of col) whose joints are in an ancestor relation AND of which at least one is an
// extra source; the deeper source supplies the moment contractions, the other one alpha / B (weights are folded into the
// per-slot tables, a record's weight word stays 1).  Entries with many terms are split into runs of at most kTermCap terms:
// run 0 stores to the entry itself, every further run to a private partial cell that one thread adds to the entry
// afterwards, in a fixed order (the combine list).
constexpr size_t kTermCap = 8; // = the records one trip of the kernels' loop consumes
struct TermRuns {
  struct Term {
    uint32_t deep, anc; // slots
  };
  struct Entry {
    int32_t dest; // tileAddress(row, col)
    std::vector<Term> terms;
  };
  struct Run {
    int32_t dest; // >= 0: float offset in the tile region ; < 0: -(cell + 1) partial cell
    size_t entry, first, count;
  };
  std::vector<Entry> entries;
  std::vector<Run> runs;
  std::vector<int32_t> comb; // three words per split entry: its dest, its first partial cell, its cells
  int32_t numCells = 0;
};
// MMX_ERR_UNSUPPORTED "more than 4095 column sources" (a record packs a slot into 12 bits) and "too many split H entries for
// the partial-cell scratch" (the kernels park the cells in a first-moment array: 7 floats per joint)
int32_t buildTermRuns(const FusedTables& f, const SlotTables& s, int32_t J, TermRuns& out, std::string& err);
// Longest-processing-time-first assignment of the runs to `threads` threads (deterministic): 256 for the one-launch solve and
// the four-wave tree kernels, 1024 for the sixteen-wave treeNormalEquationsKernel.  A record is four words: deep | anc << 12
// | first-of-run << 24 | last-of-run << 25 | 1 << 26, the dest word (bit 30: a partial cell), the weight's bits, 0.  A
// thread's records are stored interleaved (record k of thread t at [k * threads + t]) so that a wave reads them coalesced.
// Returns the rounds, a multiple of 8 (`inter` holds at least 8).
size_t dealTermRuns(const TermRuns& r, int threads, std::vector<uint32_t>& inter);

// Limits per solve column (limStart / limOf), and the limits that share an off-diagonal entry of H: per tile-region offset
// in ascending order (pairDest) its limits (pairStart / pairLim) and its (row, col) solve columns (pairCols, limitPairs).
struct LimitTables {
  std::vector<int32_t> limStart, limOf, pairDest, pairStart, pairLim, pairCols;
  std::vector<std::pair<int32_t, int32_t>> limitPairs;
};
LimitTables buildLimitTables(const mmx_rig_desc* d, const std::vector<mmx_parameter_limit>& limits, const std::vector<int32_t>& solveList);

// Solve list of the explicit-Jacobian solver: an enabled parameter none of whose joint-parameter rows has a constraint
// below it has a zero column in J, so its step is 0 (H_pp = lambda, g_p = 0) and it can leave the dense system -- exactly,
// like the fused kernel's solve list.  Forced parameters (StructureLists::force) stay.  In elimination order; `sorted` is the
// same set in index order (the double solve follows the reference's column order).  With nothing to solve for, the plain
// system is kept (all steps are zero).
struct ExplicitSolveLists {
  std::vector<int32_t> list, sorted;
};
ExplicitSolveLists buildExplicitSolveLists(const mmx_rig_desc* d, const HostTables& t, const ProblemTopology& p, const std::vector<uint8_t>& force);

// Tile structure of the wide solve's factor: entry (row, col) of H can be non-zero when a source joint of the one column is
// an ancestor-or-self of a source joint of the other (their columns of J overlap only then) or when a limit couples the two
// parameters.  The further joint error functions / ellipsoid limits (GT of them: rows over two joint chains) and systems the
// tree kernels do not take keep the dense structure.
bool tileStructureDense(const FusedTables& f, const std::vector<int32_t>& explicitList, int32_t GT);
std::vector<uint8_t> buildRelatedness(const mmx_rig_desc* d, const FusedTables& f, const std::vector<std::pair<int32_t, int32_t>>& limitPairs);
// The device array of a TileMasks: [32] row masks, [32] column masks, [32] first slot of block column i in the column-compact
// numbering; from [96] the tile in every slot, I | k << 8 (the resident kernels' load lists), then the level schedule.
std::vector<uint32_t> packTileMasks(const TileMasks& m);

// The live-joint view's tables: everything the solve kernels index by joint or by DFS position, REMAPPED from the full
// tables (solve list, elimination order, term records and tile structure stay as they are).
struct CompactRig { // the rig over the live joints
  std::vector<int32_t> parent, ptOuter, ptInner;
  std::vector<float> preRot, offset, ptValue, ptOffsets;
};
CompactRig buildCompactRig(const mmx_rig_desc* d, const LiveJoints& lj);
// Levels and the DFS interval of every live joint in the compact numbering: a live joint's ancestors are live, so its level
// is the full rig's, and the live positions keep their order (rank among the live positions).
struct CompactOrder {
  std::vector<int32_t> levelStart, levelOrder; // [numLevels + 1], [numLive]
  std::vector<int32_t> tin, tout; // [numLive]
  std::vector<int32_t> posOf; // [J] full DFS position -> live position, -1 for a dead one
};
CompactOrder buildCompactOrder(const HostTables& t, const FusedTables& f, const LiveJoints& lj);
struct LiveView {
  CompactRig rig;
  CompactOrder order;
  RigDerived derived;
  JointTables joints;
  std::vector<mmx_parameter_limit> limits; // joint-parameter rows renumbered
  std::vector<int32_t> subSize, dfsJoint; // [numLive] by live DFS position
  std::vector<int32_t> loadedPos;
  std::vector<int32_t> posUnitStart; // [numLive + 1]; indexes the FULL posUnits (a dead position carries no unit)
  std::vector<ColumnSource> slots; // pad and dead slots: weight as it was, empty interval
};
LiveView buildLiveView(
    const mmx_rig_desc* d, const HostTables& t, const FusedTables& f, const ProblemTopology& p, const LiveJoints& lj,
    const std::vector<ColumnSource>& slots);
#pragma GCC visibility pop

} // namespace mmx
