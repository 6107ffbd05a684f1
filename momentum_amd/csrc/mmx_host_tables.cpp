// mmx_host_tables.cpp -- see mmx_host_tables.hpp.  Pure host C++17, integer bookkeeping only.
#include "mmx_host_tables.hpp"

#include <algorithm>
#include <cstring>
#include <map>

namespace mmx {

int32_t validateRigDesc(const mmx_rig_desc* d, std::string& err) {
  if (d == nullptr) {
    err = "rig descriptor is null";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  const int32_t J = d->num_joints, P = d->num_params;
  if (J <= 0 || P <= 0) {
    err = "rig needs at least one joint and one model parameter";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  if (J > 32767) {
    err = "num_joints exceeds 32767 (joint and level indices are packed into 16 bits on the device)";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  if (P > MMX_MAX_MODEL_PARAMS) {
    err = "num_params exceeds kMaxModelParams (2048)";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  if (!d->parent || !d->pre_rotation || !d->translation_offset || !d->pt_outer || !d->pt_inner || !d->pt_value) {
    err = "rig descriptor has a null array";
    return MMX_ERR_INVALID_ARGUMENT;
  }
  for (int32_t j = 0; j < J; ++j) {
    // Skeleton invariant (momentum/character/skeleton.cpp:16-22): parents precede children
    if (d->parent[j] != MMX_INVALID_PARENT && (d->parent[j] < 0 || d->parent[j] >= j)) {
      err = "joint " + std::to_string(j) + " has parent " + std::to_string(d->parent[j]) +
          ": joints must be listed parent-before-child";
      return MMX_ERR_INVALID_ARGUMENT;
    }
  }
  const int32_t R = MMX_PARAMS_PER_JOINT * J;
  if (d->pt_outer[0] != 0) {
    err = "pt_outer[0] must be 0";
    return MMX_ERR_SIZE_MISMATCH;
  }
  for (int32_t r = 0; r < R; ++r) {
    if (d->pt_outer[r + 1] < d->pt_outer[r]) {
      err = "pt_outer must be non-decreasing";
      return MMX_ERR_SIZE_MISMATCH;
    }
  }
  const int32_t nnz = d->pt_outer[R];
  for (int32_t k = 0; k < nnz; ++k) {
    if (d->pt_inner[k] < 0 || d->pt_inner[k] >= P) {
      err = "parameter-transform column index out of range (transform.cols() != num_params)";
      return MMX_ERR_SIZE_MISMATCH;
    }
  }
  return MMX_OK;
}

int32_t buildHostTables(const mmx_rig_desc* d, const uint8_t* enabled, HostTables& t, std::string& err) {
  const int32_t rc = validateRigDesc(d, err);
  if (rc != MMX_OK) {
    return rc;
  }
  const int32_t J = d->num_joints, P = d->num_params, R = MMX_PARAMS_PER_JOINT * J;
  t.J = J;
  t.P = P;

  // ---- levels (parents precede children, so one forward sweep suffices)
  t.level.assign(J, 0);
  int32_t maxLevel = 0;
  for (int32_t j = 0; j < J; ++j) {
    t.level[j] = d->parent[j] < 0 ? 0 : t.level[d->parent[j]] + 1;
    maxLevel = std::max(maxLevel, t.level[j]);
  }
  t.levelStart.assign(maxLevel + 2, 0);
  for (int32_t j = 0; j < J; ++j) {
    t.levelStart[t.level[j] + 1]++;
  }
  for (int32_t l = 0; l <= maxLevel; ++l) {
    t.levelStart[l + 1] += t.levelStart[l];
  }
  t.levelOrder.assign(J, 0);
  {
    std::vector<int32_t> cursor(t.levelStart.begin(), t.levelStart.end() - 1);
    for (int32_t j = 0; j < J; ++j) { // ascending j keeps (level, index) order
      t.levelOrder[cursor[t.level[j]]++] = j;
    }
  }

  // ---- DFS pre-order intervals.  Subtree sizes by a backward sweep, then tin by a forward sweep
  // that hands each child the next free slot of its parent (children in index order).
  std::vector<int32_t> size(J, 1), nextSlot(J, 0);
  for (int32_t j = J - 1; j >= 0; --j) {
    if (d->parent[j] >= 0) {
      size[d->parent[j]] += size[j];
    }
  }
  t.tin.assign(J, 0);
  t.tout.assign(J, 0);
  int32_t rootCursor = 0;
  for (int32_t j = 0; j < J; ++j) {
    const int32_t p = d->parent[j];
    if (p < 0) {
      t.tin[j] = rootCursor;
      rootCursor += size[j];
    } else {
      t.tin[j] = nextSlot[p];
    }
    nextSlot[j] = t.tin[j] + 1;
    if (p >= 0) {
      nextSlot[p] = t.tin[j] + size[j];
    }
    t.tout[j] = t.tin[j] + size[j];
  }

  // ---- enabled set
  t.enabled.assign(P, 1);
  if (enabled != nullptr) {
    for (int32_t p = 0; p < P; ++p) {
      t.enabled[p] = enabled[p] ? 1 : 0;
    }
  }
  // GaussNewtonSolverT::updateEnabledParameters (gauss_newton_solver.cpp:57-66)
  t.enabledList.clear();
  t.fullToSubset.assign(P, -1);
  for (int32_t p = 0; p < P; ++p) {
    if (t.enabled[p]) {
      t.fullToSubset[p] = int32_t(t.enabledList.size());
      t.enabledList.push_back(p);
    }
  }
  // ---- elimination order: joints in post-order (children before their parent, smaller subtrees first, ties by index);
  // a parameter sits where the LAST of the joints it drives does (a shared parameter joins the highest of its joints)
  {
    std::vector<std::vector<int32_t>> children(J);
    std::vector<int32_t> roots;
    for (int32_t j = 0; j < J; ++j) {
      (d->parent[j] >= 0 ? children[d->parent[j]] : roots).push_back(j);
    }
    auto bySize = [&](int32_t a, int32_t b) { return size[a] != size[b] ? size[a] < size[b] : a < b; };
    std::stable_sort(roots.begin(), roots.end(), bySize);
    for (auto& c : children) {
      std::stable_sort(c.begin(), c.end(), bySize);
    }
    std::vector<int32_t> postPos(J, 0), stack, cursor(J, 0);
    int32_t next = 0;
    for (int32_t r : roots) {
      stack.push_back(r);
      while (!stack.empty()) {
        const int32_t j = stack.back();
        if (cursor[j] < int32_t(children[j].size())) {
          stack.push_back(children[j][cursor[j]++]);
        } else {
          postPos[j] = next++;
          stack.pop_back();
        }
      }
    }
    std::vector<int32_t> key(P, J); // parameters that drive no joint: last, by index
    for (int32_t r = 0; r < R; ++r) {
      for (int32_t k = d->pt_outer[r]; k < d->pt_outer[r + 1]; ++k) {
        const int32_t p = d->pt_inner[k], pos = postPos[r / MMX_PARAMS_PER_JOINT];
        key[p] = key[p] == J ? pos : std::max(key[p], pos);
      }
    }
    t.eliminationList = t.enabledList;
    std::stable_sort(t.eliminationList.begin(), t.eliminationList.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
  }
  // ParameterTransformT::computeActiveJointParams (parameter_transform.cpp:97-107)
  t.activeJointParams.assign(R, 0);
  for (int32_t r = 0; r < R; ++r) {
    for (int32_t k = d->pt_outer[r]; k < d->pt_outer[r + 1]; ++k) {
      if (t.enabled[d->pt_inner[k]]) {
        t.activeJointParams[r] = 1;
      }
    }
  }

  // ---- CSC view of the enabled entries: column p lists its (joint, dof, weight) sources in
  // ascending joint-parameter row order.  A zero stored value is kept (the reference multiplies by
  // it too).  Rows of a disabled column are dropped here, which is the
  // enabledParameters_.test(inner[k]) test of joint_error_function-inl.h:257,273,286.
  std::vector<int32_t> count(P + 1, 0);
  for (int32_t r = 0; r < R; ++r) {
    for (int32_t k = d->pt_outer[r]; k < d->pt_outer[r + 1]; ++k) {
      if (t.enabled[d->pt_inner[k]]) {
        count[d->pt_inner[k] + 1]++;
      }
    }
  }
  t.colStart.assign(P + 1, 0);
  for (int32_t p = 0; p < P; ++p) {
    t.colStart[p + 1] = t.colStart[p] + count[p + 1];
  }
  t.colSources.assign(t.colStart[P], ColumnSource{});
  std::vector<int32_t> cursor(t.colStart.begin(), t.colStart.end() - 1);
  for (int32_t r = 0; r < R; ++r) {
    const int32_t joint = r / MMX_PARAMS_PER_JOINT, dof = r % MMX_PARAMS_PER_JOINT;
    for (int32_t k = d->pt_outer[r]; k < d->pt_outer[r + 1]; ++k) {
      const int32_t p = d->pt_inner[k];
      if (!t.enabled[p]) {
        continue;
      }
      ColumnSource& s = t.colSources[cursor[p]++];
      s.joint = joint;
      s.dof = dof;
      s.tin = t.tin[joint];
      s.tout = t.tout[joint];
      s.parent = d->parent[joint];
      s.weight = d->pt_value[k];
    }
  }
  t.maxColSources = 0;
  for (int32_t p = 0; p < P; ++p) {
    t.maxColSources = std::max(t.maxColSources, t.colStart[p + 1] - t.colStart[p]);
  }
  // column program of the J-assembly kernel: single-source ROTATION columns (the bulk of any rig)
  // go to the record list grouped by joint; every other non-empty column takes the generic path
  t.jacRecs.clear();
  t.multiCols.clear();
  t.zeroCols.clear();
  for (int32_t p = 0; p < P; ++p) {
    const int32_t cnt = t.colStart[p + 1] - t.colStart[p];
    if (cnt == 0) {
      t.zeroCols.push_back(p);
      continue;
    }
    const ColumnSource& s = t.colSources[t.colStart[p]];
    if (cnt == 1 && s.dof >= 3 && s.dof < 6) {
      t.jacRecs.push_back(JacRec{s.joint, s.dof, p, s.tin, s.tout, s.parent, s.weight, 1});
    } else {
      t.multiCols.push_back(p);
    }
  }
  std::stable_sort(t.jacRecs.begin(), t.jacRecs.end(), [](const JacRec& a, const JacRec& b) {
    return a.joint != b.joint ? a.joint < b.joint : a.dof < b.dof;
  });
  // pad to a multiple of 4 with copies of the last record (re-writing a column with the same
  // values is idempotent)
  while (!t.jacRecs.empty() && t.jacRecs.size() % 4 != 0) {
    t.jacRecs.push_back(t.jacRecs.back());
  }
  return MMX_OK;
}

StateBackwardTables buildStateBackwardTables(const HostTables& t) {
  StateBackwardTables s;
  const int32_t J = t.J;
  s.dfsJoint.assign(size_t(J), 0);
  s.subSize.assign(size_t(J), 1);
  s.loadedPos.resize(size_t(J));
  for (int32_t j = 0; j < J; ++j) {
    s.dfsJoint[size_t(t.tin[size_t(j)])] = j;
    s.subSize[size_t(t.tin[size_t(j)])] = t.tout[size_t(j)] - t.tin[size_t(j)];
    s.loadedPos[size_t(j)] = j;
  }
  s.jointPos = t.tin;
  s.colStart = t.colStart; // (every parameter enabled: no entry of the transform was dropped)
  s.colSources = t.colSources;
  return s;
}

int32_t buildFusedTables(
    const mmx_rig_desc* d,
    const HostTables& t,
    int32_t Kp,
    const int32_t* posParent,
    int32_t Ko,
    const int32_t* oriParent,
    const uint8_t* forceSolve,
    const std::vector<int32_t>* unionPos,
    const std::vector<int32_t>* unionOri,
    FusedTables& f,
    std::string& err) {
  const int32_t J = t.J, P = t.P;
  f.U = Kp + 3 * Ko;
  f.dfsJoint.assign(J, 0);
  f.subSize.assign(J, 1);
  for (int32_t j = 0; j < J; ++j) {
    f.dfsJoint[t.tin[j]] = j;
    f.subSize[t.tin[j]] = t.tout[j] - t.tin[j];
  }
  f.maxDepth = 0;
  for (int32_t j = 0; j < J; ++j) {
    f.maxDepth = std::max(f.maxDepth, t.level[j]);
  }
  f.unitJoint.assign(size_t(std::max(f.U, 1)), 0);
  for (int32_t c = 0; c < Kp; ++c) {
    f.unitJoint[c] = posParent[c];
  }
  for (int32_t c = 0; c < Ko; ++c) {
    for (int k = 0; k < 3; ++k) {
      f.unitJoint[Kp + 3 * c + k] = oriParent[c];
    }
  }
  // units per DFS position (ascending unit index within a joint: deterministic summation order)
  f.posUnitStart.assign(J + 1, 0);
  for (int32_t u = 0; u < f.U; ++u) {
    f.posUnitStart[t.tin[f.unitJoint[u]] + 1]++;
  }
  for (int32_t k = 0; k < J; ++k) {
    f.posUnitStart[k + 1] += f.posUnitStart[k];
  }
  f.posUnits.assign(size_t(std::max(f.U, 1)), 0);
  {
    std::vector<int32_t> cur(f.posUnitStart.begin(), f.posUnitStart.end() - 1);
    for (int32_t u = 0; u < f.U; ++u) {
      f.posUnits[cur[t.tin[f.unitJoint[u]]]++] = u;
    }
  }
  // a joint is "loaded" if some unit sits in its subtree (in some element of the batch, when the
  // constraint parents are per instance)
  std::vector<uint8_t> loaded(J, 0);
  auto markLoaded = [&](int32_t a) {
    while (a >= 0 && !loaded[a]) {
      loaded[a] = 1;
      a = d->parent[a];
    }
  };
  for (int32_t u = 0; u < f.U; ++u) {
    markLoaded(f.unitJoint[u]);
  }
  for (const std::vector<int32_t>* lst : {unionPos, unionOri}) {
    if (lst != nullptr) {
      for (int32_t j : *lst) {
        markLoaded(j);
      }
    }
  }
  // Orientation constraints only see rotation dofs, position constraints see all: a column is
  // structurally non-zero iff it has a source (a,dof) with a unit below a that the dof acts on.
  std::vector<uint8_t> hasPoint(J, 0);
  auto markPoint = [&](int32_t a) {
    while (a >= 0 && !hasPoint[a]) {
      hasPoint[a] = 1;
      a = d->parent[a];
    }
  };
  for (int32_t c = 0; c < Kp; ++c) {
    markPoint(posParent[c]);
  }
  if (unionPos != nullptr) {
    for (int32_t j : *unionPos) {
      markPoint(j);
    }
  }
  f.solveList.clear();
  f.srcStart.assign(1, 0);
  f.srcs.clear();
  f.structNonZero.assign(size_t(P), 0);
  for (int32_t p : t.eliminationList) {
    bool nz = false;
    for (int32_t e = t.colStart[p]; e < t.colStart[p + 1]; ++e) {
      const ColumnSource& s = t.colSources[e];
      const bool rot = s.dof >= 3 && s.dof < 6;
      if (rot ? loaded[s.joint] : hasPoint[s.joint]) {
        nz = true;
      }
    }
    f.structNonZero[size_t(p)] = nz ? 1 : 0;
    if (!nz && !(forceSolve != nullptr && forceSolve[p] != 0)) {
      continue;
    }
    f.solveList.push_back(p);
    // only the sources that can move a unit: a rotation dof with a unit in its joint's subtree, a
    // translation / scale dof with a POINT there (the others have zero moments below them, so every term
    // they take part in is exactly zero)
    for (int32_t e = t.colStart[p]; nz && e < t.colStart[p + 1]; ++e) {
      const ColumnSource& s = t.colSources[e];
      const bool rot = s.dof >= 3 && s.dof < 6;
      if (rot ? loaded[s.joint] : hasPoint[s.joint]) {
        f.srcs.push_back(s);
      }
    }
    f.srcStart.push_back(int32_t(f.srcs.size()));
  }
  (void)err;
  return MMX_OK;
}

void buildLiveJoints(const int32_t* parent, int32_t J, const int32_t* joints, int32_t n, LiveJoints& out) {
  out.live.assign(size_t(J), 0);
  int32_t count = 0;
  for (int32_t i = 0; i < n; ++i) {
    for (int32_t a = joints[i]; a >= 0 && a < J && !out.live[size_t(a)]; a = parent[a]) {
      out.live[size_t(a)] = 1;
      ++count;
    }
  }
  if (count == 0) { // nothing referenced: nothing to prune by
    out.live.assign(size_t(J), 1);
    count = J;
  }
  out.numLive = count;
  out.compactOf.assign(size_t(J), -1);
  out.fullOf.clear();
  for (int32_t j = 0; j < J; ++j) {
    if (out.live[size_t(j)]) {
      out.compactOf[size_t(j)] = int32_t(out.fullOf.size());
      out.fullOf.push_back(j);
    }
  }
}

TileMasks eliminationTileMasks(int32_t n, const std::vector<uint8_t>& related, bool dense) {
  TileMasks m;
  const int32_t NB = (n + 15) / 16;
  m.NB = NB;
  if (NB > 32) {
    return m;
  }
  for (int32_t I = 0; I < NB; ++I) {
    m.rowMask[I] = dense ? (I == 31 ? 0xffffffffu : ((1u << (I + 1)) - 1u)) : (1u << I);
  }
  if (!dense) {
    for (int32_t row = 0; row < n; ++row) {
      for (int32_t col = 0; col < row; ++col) {
        if (related[size_t(row) * size_t(n) + size_t(col)]) {
          m.rowMask[row >> 4] |= 1u << (col >> 4);
        }
      }
    }
    for (int32_t k = 0; k < NB; ++k) { // fill: the rows that hold a tile in column k become mutually coupled
      for (int32_t a = k + 1; a < NB; ++a) {
        if (!(m.rowMask[a] >> k & 1u)) {
          continue;
        }
        for (int32_t bb = k + 1; bb <= a; ++bb) {
          if (m.rowMask[bb] >> k & 1u) {
            m.rowMask[a] |= 1u << bb;
          }
        }
      }
    }
  }
  for (int32_t I = 0; I < NB; ++I) {
    for (int32_t k = 0; k <= I; ++k) {
      if (m.rowMask[I] >> k & 1u) {
        m.colMask[k] |= 1u << I;
        m.tiles.push_back(I | (k << 8));
        const uint32_t below = k == 0 ? 0u : ((1u << k) - 1u);
        m.products += __builtin_popcount(m.rowMask[I] & m.rowMask[k] & below);
      }
    }
  }
  // level schedule (TileMasks::levelSteps)
  {
    int32_t level[32] = {};
    int32_t maxLevel = -1;
    for (int32_t k = 0; k < NB; ++k) {
      int32_t lv = 0;
      for (int32_t j = 0; j < k; ++j) {
        if (m.rowMask[k] >> j & 1u) {
          lv = std::max(lv, level[j] + 1);
        }
      }
      level[k] = lv;
      maxLevel = std::max(maxLevel, lv);
    }
    std::vector<int32_t> steps;
    for (int32_t lv = 0; lv <= maxLevel; ++lv) {
      int32_t used = 0, inStep = 0;
      auto flush = [&]() {
        while (inStep > 0 && inStep < 4) {
          steps.push_back(-1);
          ++inStep;
        }
        used = 0, inStep = 0;
      };
      // the widest panels first: they take the low waves, the narrow ones fill up
      std::vector<int32_t> cols;
      for (int32_t k = 0; k < NB; ++k) {
        if (level[k] == lv) {
          cols.push_back(k);
        }
      }
      std::stable_sort(cols.begin(), cols.end(), [&](int32_t a, int32_t b2) { return __builtin_popcount(m.colMask[a]) > __builtin_popcount(m.colMask[b2]); });
      for (int32_t k : cols) {
        const int32_t nt = __builtin_popcount(m.colMask[k]);
        const int32_t rowsBelow = 16 * (nt - 1);
        if (rowsBelow > 192) { // the whole workgroup (tiledPanelFactor's tail substitution takes the rows beyond 208)
          flush();
          steps.push_back(k | (0 << 8) | (0xf << 12));
          inStep = 1;
          flush();
          continue;
        }
        const int32_t nw = std::max(1, (rowsBelow + 47) / 48);
        if (used + nw > 4 || inStep == 4) {
          flush();
        }
        steps.push_back(k | (used << 8) | (nw << 12));
        used += nw, ++inStep;
      }
      flush();
    }
    m.levelSteps.clear();
    m.levelSteps.push_back(int32_t(steps.size() / 4));
    m.levelSteps.insert(m.levelSteps.end(), steps.begin(), steps.end());
  }
  return m;
}

bool buildF64AssemblyListHost(
    const HostTables& t, const std::vector<int32_t>& solveList, const int32_t* posParent, int32_t Kp, const int32_t* oriParent, int32_t Ko,
    int32_t uc, F64AssemblyListHost& out) {
  const int32_t n = int32_t(solveList.size()), U = Kp + 3 * Ko;
  std::vector<int32_t> prefix(size_t(n) + 1, 0);
  for (int32_t c = 0; c < n; ++c) {
    const int32_t p = solveList[size_t(c)];
    prefix[size_t(c) + 1] = prefix[size_t(c)] + (t.colStart[size_t(p) + 1] - t.colStart[size_t(p)]);
  }
  std::vector<int32_t> unitTin(size_t(std::max(U, 1)));
  for (int32_t c = 0; c < Kp; ++c) {
    unitTin[size_t(c)] = t.tin[size_t(posParent[size_t(c)])];
  }
  for (int32_t c = 0; c < Ko; ++c) {
    for (int k = 0; k < 3; ++k) {
      unitTin[size_t(Kp + 3 * c + k)] = t.tin[size_t(oriParent[size_t(c)])];
    }
  }
  out.groups.clear(), out.extra.clear(), out.chunkStart.clear();
  std::vector<int32_t> blockMasks;
  for (int32_t u0 = 0; u0 < U; u0 += uc) {
    out.chunkStart.push_back(int32_t(out.groups.size() / 2));
    blockMasks.push_back(0);
    for (int32_t u = u0; u < std::min(U, u0 + uc); ++u) {
      const bool isPoint = u < Kp;
      for (int32_t c = 0; c < n; ++c) {
        const int32_t p = solveList[size_t(c)];
        int32_t count = 0, first = -1;
        const size_t extraAt = out.extra.size();
        for (int32_t e = t.colStart[size_t(p)]; e < t.colStart[size_t(p) + 1]; ++e) {
          const ColumnSource& cs = t.colSources[size_t(e)];
          const bool rot = cs.dof >= 3 && cs.dof < 6;
          if (cs.tin <= unitTin[size_t(u)] && unitTin[size_t(u)] < cs.tout && (rot || isPoint)) {
            const int32_t k = prefix[size_t(c)] + (e - t.colStart[size_t(p)]);
            if (count == 0) {
              first = k;
            }
            out.extra.push_back(k);
            ++count;
          }
        }
        if (count == 0) {
          continue;
        }
        if (count > 8191) {
          return false;
        }
        if (count == 1) {
          out.extra.resize(extraAt); // (a single source rides in the group word)
        }
        blockMasks.back() |= int32_t(1u << std::min(c >> 4, 31)); // (blocks beyond 31 share the last bit: n <= 208 has 13)
        out.groups.push_back(uint32_t(c) | uint32_t(u - u0) << 12 | uint32_t(count) << 18);
        out.groups.push_back(uint32_t(count == 1 ? first : int32_t(extraAt)));
      }
    }
  }
  out.chunkStart.push_back(int32_t(out.groups.size() / 2));
  out.chunkStart.insert(out.chunkStart.end(), blockMasks.begin(), blockMasks.end());
  return true;
}

// ---- problem tables (see the header)

std::vector<int32_t> limitParameters(const mmx_rig_desc* d, const mmx_parameter_limit& lm) {
  std::vector<int32_t> out;
  auto add = [&](int32_t p) {
    if (std::find(out.begin(), out.end(), p) == out.end()) {
      out.push_back(p);
    }
  };
  auto addRow = [&](int32_t row) {
    for (int32_t k = d->pt_outer[size_t(row)]; k < d->pt_outer[size_t(row) + 1]; ++k) {
      add(d->pt_inner[size_t(k)]);
    }
  };
  switch (lm.type) {
    case MMX_LIMIT_MINMAX:
      add(lm.index0);
      break;
    case MMX_LIMIT_LINEAR:
    case MMX_LIMIT_HALFPLANE:
      add(lm.index0);
      add(lm.index1);
      break;
    case MMX_LIMIT_MINMAX_JOINT:
      addRow(lm.index0);
      break;
    case MMX_LIMIT_LINEAR_JOINT:
      addRow(lm.index1);
      addRow(lm.index0);
      break;
    default:
      break;
  }
  return out;
}

RigDerived deriveRigTables(
    int32_t J, int32_t P, const std::vector<int32_t>& parent, const std::vector<int32_t>& ptOuter, const std::vector<int32_t>& ptInner,
    const std::vector<float>& ptValue, int32_t numLevels) {
  RigDerived o;
  const int32_t R = MMX_PARAMS_PER_JOINT * J;
  o.ell.assign(size_t(R) * 4, 0);
  o.jumpParent.assign(size_t(J), 0);
  for (int32_t row = 0; row < R; ++row) {
    const int32_t k0 = ptOuter[size_t(row)], k1 = ptOuter[size_t(row) + 1];
    if (k1 - k0 > 2) {
      o.ellOk = false;
      break;
    }
    for (int s = 0; s < 2; ++s) {
      int32_t idx = -1, bits = 0;
      if (k0 + s < k1) {
        idx = ptInner[size_t(k0 + s)];
        std::memcpy(&bits, &ptValue[size_t(k0 + s)], 4);
      }
      o.ell[4 * size_t(row) + 2 * s] = idx;
      o.ell[4 * size_t(row) + 2 * s + 1] = bits;
    }
  }
  for (int32_t j = 0; j < J; ++j) {
    o.jumpParent[size_t(j)] = ((parent[size_t(j)] + 1) << 16) | (parent[size_t(j)] + 1);
  }
  if (R < 65536 && P <= 65535) { // (every field of a record is an unsigned 16-bit number: row, rows to the next record, first column, entries)
    std::vector<int32_t> rows;
    for (int32_t row = 0; row < R; ++row) {
      if (ptOuter[size_t(row) + 1] > ptOuter[size_t(row)]) {
        rows.push_back(row);
      }
    }
    for (size_t t = 0; t < rows.size(); ++t) {
      const int32_t row = rows[t], next = t + 1 < rows.size() ? rows[t + 1] : R;
      const int32_t k0 = ptOuter[size_t(row)], cnt = ptOuter[size_t(row) + 1] - k0;
      if (cnt > 65535 || next - row > 65535) { // (does not fit: no records at all, the kernels walk the CSR)
        o.rowRec.clear();
        break;
      }
      int32_t bits = 0;
      std::memcpy(&bits, &ptValue[size_t(k0)], 4);
      o.rowRec.insert(o.rowRec.end(), {row | ((next - row) << 16), ptInner[size_t(k0)] | (cnt << 16), bits, k0});
    }
  }
  while ((1 << o.jumpRounds) < numLevels) {
    ++o.jumpRounds;
  }
  return o;
}

std::vector<int32_t> referencedJoints(const ProblemTopology& p) {
  std::vector<int32_t> ref(p.posParent);
  ref.insert(ref.end(), p.oriParent.begin(), p.oriParent.end());
  for (const ProblemTopology::Block& h : p.blocks) {
    ref.insert(ref.end(), h.parent.begin(), h.parent.end());
    ref.insert(ref.end(), h.parentB.begin(), h.parentB.end());
  }
  for (const mmx_ellipsoid_limit& e : p.ellipsoids) {
    ref.push_back(e.parent);
    ref.push_back(e.ellipsoid_parent);
  }
  for (const mmx_parameter_limit& lm : p.limits) {
    if (lm.type == MMX_LIMIT_MINMAX_JOINT || lm.type == MMX_LIMIT_LINEAR_JOINT) {
      ref.push_back(lm.index0 / MMX_PARAMS_PER_JOINT);
    }
    if (lm.type == MMX_LIMIT_LINEAR_JOINT) {
      ref.push_back(lm.index1 / MMX_PARAMS_PER_JOINT);
    }
  }
  return ref;
}

JointTables buildJointTables(const ProblemTopology& p, const int32_t* compactOf, const std::vector<int32_t>& tin, const std::vector<int32_t>& tout) {
  JointTables o;
  auto cj = [&](int32_t j) { return j < 0 || compactOf == nullptr ? j : compactOf[size_t(j)]; };
  const int32_t U = p.U();
  o.unitJoint.assign(size_t(std::max(U, 1)), 0);
  o.unitTin.assign(size_t(std::max(U, 1)), 0);
  for (int32_t c = 0; c < p.Kp; ++c) {
    o.unitJoint[size_t(c)] = cj(p.posParent[size_t(c)]);
  }
  for (int32_t c = 0; c < p.Ko; ++c) {
    for (int k = 0; k < 3; ++k) {
      o.unitJoint[size_t(p.Kp + 3 * c + k)] = cj(p.oriParent[size_t(c)]);
    }
  }
  for (int32_t u = 0; u < U; ++u) {
    o.unitTin[size_t(u)] = tin[size_t(o.unitJoint[size_t(u)])];
  }
  std::vector<int32_t> gj2, gt2;
  for (size_t i = 0; i < p.blocks.size(); ++i) {
    const ProblemTopology::Block& h = p.blocks[i];
    for (size_t c = 0; c < h.parent.size(); ++c) {
      const int32_t j = cj(h.parent[c]), j2 = h.parentB.empty() ? -1 : cj(h.parentB[c]);
      o.genJoint.push_back(j);
      o.genTin.push_back(tin[size_t(j)]);
      o.genBlock.push_back(int32_t(i));
      gj2.push_back(j2);
      gt2.push_back(j2 < 0 ? -1 : tin[size_t(j2)]);
    }
  }
  o.genJoint.insert(o.genJoint.end(), gj2.begin(), gj2.end());
  o.genTin.insert(o.genTin.end(), gt2.begin(), gt2.end());
  for (const mmx_ellipsoid_limit& e : p.ellipsoids) {
    const int32_t pj = cj(e.parent), ep = cj(e.ellipsoid_parent);
    const bool onChain = tin[size_t(ep)] <= tin[size_t(pj)] && tin[size_t(pj)] < tout[size_t(ep)];
    o.ellParent.push_back(pj);
    o.ellEllipsoidParent.push_back(ep);
    o.ellTinParent.push_back(tin[size_t(pj)]);
    o.ellTinStop.push_back(onChain ? tin[size_t(ep)] : -1);
  }
  return o;
}

namespace {
bool isFixedAxis(int32_t type) {
  return type == MMX_JC_FIXED_AXIS_DIFF || type == MMX_JC_FIXED_AXIS_COS || type == MMX_JC_FIXED_AXIS_ANGLE;
}
} // namespace

StructureLists buildStructureLists(const mmx_rig_desc* d, const ProblemTopology& p) {
  StructureLists s;
  s.force.assign(size_t(d->num_params), p.hasModel ? 1 : 0);
  for (const mmx_parameter_limit& lm : p.limits) {
    for (int32_t q : limitParameters(d, lm)) {
      s.force[size_t(q)] = 1;
    }
  }
  if (p.instPos) {
    s.structPos = p.unionPos;
  }
  if (p.instOri) {
    s.structOri = p.unionOri;
  }
  for (const ProblemTopology::Block& h : p.blocks) {
    for (int32_t j : h.parent) {
      (isFixedAxis(h.type) ? s.structOri : s.structPos).push_back(j);
    }
    s.structPos.insert(s.structPos.end(), h.parentB.begin(), h.parentB.end()); // a pair row also walks the chain above its second point
  }
  for (const mmx_ellipsoid_limit& e : p.ellipsoids) {
    s.structPos.push_back(e.parent);
  }
  return s;
}

int32_t buildProblemFusedTables(
    const mmx_rig_desc* d, const HostTables& t, const ProblemTopology& p, const StructureLists& s, FusedTables& out, std::string& err) {
  return buildFusedTables(
      d, t, p.Kp, p.posParent.data(), p.Ko, p.oriParent.data(), s.force.data(), s.structPos.empty() ? nullptr : &s.structPos,
      s.structOri.empty() ? nullptr : &s.structOri, out, err);
}

ColumnProgram buildColumnProgram(const HostTables& t, const FusedTables& f) {
  ColumnProgram o;
  for (int32_t p = 0; p < t.P; ++p) {
    const int32_t cnt = t.colStart[size_t(p) + 1] - t.colStart[size_t(p)];
    if (cnt == 0 || !f.structNonZero[size_t(p)]) {
      o.zero.push_back(p);
      continue;
    }
    const ColumnSource& cs = t.colSources[size_t(t.colStart[size_t(p)])];
    if (cnt == 1 && cs.dof >= 3 && cs.dof < 6) {
      o.recs.push_back(JacRec{cs.joint, cs.dof, p, cs.tin, cs.tout, cs.parent, cs.weight, 1});
    } else {
      o.multi.push_back(p);
    }
  }
  std::stable_sort(o.recs.begin(), o.recs.end(), [](const JacRec& a, const JacRec& b) { return a.joint != b.joint ? a.joint < b.joint : a.dof < b.dof; });
  while (!o.recs.empty() && o.recs.size() % 4 != 0) {
    o.recs.push_back(o.recs.back());
  }
  return o;
}

SlotTables buildSlotTables(const FusedTables& f, int32_t slotBlocks) {
  SlotTables o;
  for (int32_t k = 0; k + 1 < int32_t(f.posUnitStart.size()); ++k) {
    if (f.posUnitStart[size_t(k) + 1] > f.posUnitStart[size_t(k)]) {
      o.loadedPos.push_back(k);
    }
  }
  const ColumnSource pad{0, 3, 0, 0, -1, 0.f};
  const int32_t NPs = 16 * slotBlocks, ncol = int32_t(f.solveList.size());
  o.slotBase = NPs;
  o.slots.assign(size_t(NPs), pad);
  o.xStart.assign(size_t(NPs) + 1, 0);
  o.slotOf.assign(f.srcs.size(), -1);
  for (int32_t c = 0; c < ncol; ++c) {
    o.xStart[size_t(c)] = int32_t(o.slots.size()) - NPs;
    for (int32_t e = f.srcStart[size_t(c)]; e < f.srcStart[size_t(c) + 1]; ++e) {
      if (e == f.srcStart[size_t(c)]) {
        o.slots[size_t(c)] = f.srcs[size_t(e)];
        o.slotOf[size_t(e)] = c;
      } else {
        o.slotOf[size_t(e)] = int32_t(o.slots.size());
        o.slots.push_back(f.srcs[size_t(e)]);
      }
    }
  }
  for (int32_t c = ncol; c <= NPs; ++c) {
    o.xStart[size_t(c)] = int32_t(o.slots.size()) - NPs;
  }
  while (o.slots.size() % 4 != 0) {
    o.slots.push_back(pad);
  }
  return o;
}

int32_t buildTermRuns(const FusedTables& f, const SlotTables& s, int32_t J, TermRuns& o, std::string& err) {
  o = TermRuns{};
  const int32_t n = int32_t(f.solveList.size());
  for (int32_t row = 0; row < n; ++row) {
    for (int32_t col = 0; col <= row; ++col) {
      TermRuns::Entry en;
      for (int32_t er = f.srcStart[size_t(row)]; er < f.srcStart[size_t(row) + 1]; ++er) {
        for (int32_t ec = f.srcStart[size_t(col)]; ec < f.srcStart[size_t(col) + 1]; ++ec) {
          if (er == f.srcStart[size_t(row)] && ec == f.srcStart[size_t(col)]) {
            continue; // primary x primary: the matrix-core pass
          }
          const ColumnSource &sa = f.srcs[size_t(er)], &sc = f.srcs[size_t(ec)];
          int32_t deep, anc;
          if (sc.tin <= sa.tin && sa.tin < sc.tout) {
            deep = s.slotOf[size_t(er)], anc = s.slotOf[size_t(ec)];
          } else if (sa.tin <= sc.tin && sc.tin < sa.tout) {
            deep = s.slotOf[size_t(ec)], anc = s.slotOf[size_t(er)];
          } else {
            continue;
          }
          en.terms.push_back(TermRuns::Term{uint32_t(deep), uint32_t(anc)});
        }
      }
      if (en.terms.empty()) {
        continue;
      }
      en.dest = tileAddress(row, col);
      o.entries.push_back(std::move(en));
    }
  }
  if (s.slots.size() >= size_t(1 << 12)) {
    err = "more than 4095 column sources";
    return MMX_ERR_UNSUPPORTED;
  }
  for (size_t e = 0; e < o.entries.size(); ++e) {
    const size_t nt = o.entries[e].terms.size();
    const size_t chunks = (nt + kTermCap - 1) / kTermCap;
    for (size_t c = 0; c < chunks; ++c) { // (chunk c >= 1 of an entry uses partial cell first + c - 1)
      const size_t first = c * kTermCap, count = std::min(kTermCap, nt - first);
      o.runs.push_back(TermRuns::Run{c == 0 ? o.entries[e].dest : -(o.numCells + int32_t(c)), e, first, count});
    }
    if (chunks > 1) {
      o.comb.insert(o.comb.end(), {o.entries[e].dest, o.numCells, int32_t(chunks - 1)});
      o.numCells += int32_t(chunks - 1);
    }
  }
  if (o.numCells > 7 * J) { // the kernels park the cells in a first-moment array: kC1 (= 7) floats per joint
    err = "too many split H entries for the partial-cell scratch";
    return MMX_ERR_UNSUPPORTED;
  }
  return MMX_OK;
}

size_t dealTermRuns(const TermRuns& r, int threads, std::vector<uint32_t>& inter) {
  std::vector<size_t> order(r.runs.size());
  for (size_t i = 0; i < order.size(); ++i) {
    order[i] = i;
  }
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return r.runs[x].count > r.runs[y].count; });
  const size_t nThreads = size_t(threads);
  std::vector<std::vector<uint32_t>> recs(nThreads); // 4 words per record
  std::vector<size_t> load(nThreads, 0);
  const float one = 1.f;
  uint32_t wbits;
  std::memcpy(&wbits, &one, 4);
  for (size_t oi : order) {
    const TermRuns::Run& rn = r.runs[oi];
    int thread = 0;
    for (int t = 1; t < threads; ++t) {
      if (load[size_t(t)] < load[size_t(thread)]) {
        thread = t;
      }
    }
    const TermRuns::Entry& en = r.entries[rn.entry];
    const uint32_t destWord = rn.dest >= 0 ? uint32_t(rn.dest) : (1u << 30) | uint32_t(-rn.dest - 1);
    for (size_t i = 0; i < rn.count; ++i) {
      const TermRuns::Term& tm = en.terms[rn.first + i];
      uint32_t x = tm.deep | (tm.anc << 12) | (1u << 26);
      if (i == 0) {
        x |= 1u << 24;
      }
      if (i + 1 == rn.count) {
        x |= 1u << 25;
      }
      recs[size_t(thread)].insert(recs[size_t(thread)].end(), {x, destWord, wbits, 0u});
    }
    load[size_t(thread)] += rn.count;
  }
  size_t rounds = 0;
  for (const auto& rc : recs) {
    rounds = std::max(rounds, rc.size() / 4);
  }
  rounds = (rounds + 7) & ~size_t(7); // the kernels consume 8 records per trip
  inter.assign(std::max<size_t>(rounds, 8) * nThreads * 4, 0u);
  for (size_t t = 0; t < nThreads; ++t) {
    for (size_t k = 0; k < recs[t].size() / 4; ++k) {
      for (size_t w = 0; w < 4; ++w) {
        inter[(k * nThreads + t) * 4 + w] = recs[t][4 * k + w];
      }
    }
  }
  return rounds;
}

LimitTables buildLimitTables(const mmx_rig_desc* d, const std::vector<mmx_parameter_limit>& limits, const std::vector<int32_t>& solveList) {
  LimitTables o;
  const int32_t n = int32_t(solveList.size());
  std::vector<int32_t> colOf(size_t(d->num_params), -1);
  for (int32_t c = 0; c < n; ++c) {
    colOf[size_t(solveList[size_t(c)])] = c;
  }
  std::vector<std::vector<int32_t>> per(size_t(std::max(n, 1)));
  std::map<int32_t, std::vector<int32_t>> pairs; // tile-region offset -> limits
  std::map<int32_t, std::pair<int32_t, int32_t>> pairColumns;
  for (size_t l = 0; l < limits.size(); ++l) {
    std::vector<int32_t> cols;
    for (int32_t p : limitParameters(d, limits[l])) {
      if (colOf[size_t(p)] >= 0) {
        cols.push_back(colOf[size_t(p)]);
      }
    }
    for (int32_t c : cols) {
      per[size_t(c)].push_back(int32_t(l));
    }
    for (size_t x = 0; x < cols.size(); ++x) {
      for (size_t y = x + 1; y < cols.size(); ++y) {
        const int32_t row = std::max(cols[x], cols[y]), col = std::min(cols[x], cols[y]);
        const int32_t dest = tileAddress(row, col);
        pairs[dest].push_back(int32_t(l));
        pairColumns[dest] = {row, col};
      }
    }
  }
  o.limStart.assign(1, 0);
  o.pairStart.assign(1, 0);
  for (int32_t c = 0; c < n; ++c) {
    o.limOf.insert(o.limOf.end(), per[size_t(c)].begin(), per[size_t(c)].end());
    o.limStart.push_back(int32_t(o.limOf.size()));
  }
  for (const auto& kv : pairs) {
    const std::pair<int32_t, int32_t> rc = pairColumns[kv.first];
    o.pairDest.push_back(kv.first);
    o.pairCols.push_back(rc.first);
    o.pairCols.push_back(rc.second);
    o.limitPairs.push_back(rc);
    o.pairLim.insert(o.pairLim.end(), kv.second.begin(), kv.second.end());
    o.pairStart.push_back(int32_t(o.pairLim.size()));
  }
  return o;
}

ExplicitSolveLists buildExplicitSolveLists(const mmx_rig_desc* d, const HostTables& t, const ProblemTopology& p, const std::vector<uint8_t>& force) {
  const size_t J = size_t(d->num_joints);
  std::vector<uint8_t> anyBelow(J, 0), pointBelow(J, 0); // a constraint vector / a constraint POINT in the joint's subtree
  auto mark = [&](int32_t joint, bool point) {
    for (int32_t a = joint; a >= 0; a = d->parent[size_t(a)]) {
      anyBelow[size_t(a)] = 1;
      if (point) {
        pointBelow[size_t(a)] = 1;
      }
    }
  };
  for (int32_t j : p.posParent) {
    mark(j, true);
  }
  for (int32_t j : p.oriParent) {
    mark(j, false);
  }
  if (p.instPos) {
    for (int32_t j : p.unionPos) {
      mark(j, true);
    }
  }
  if (p.instOri) {
    for (int32_t j : p.unionOri) {
      mark(j, false);
    }
  }
  for (const ProblemTopology::Block& h : p.blocks) {
    for (int32_t j : h.parent) {
      mark(j, !isFixedAxis(h.type));
    }
    for (int32_t j : h.parentB) {
      mark(j, true);
    }
  }
  for (const mmx_ellipsoid_limit& e : p.ellipsoids) {
    mark(e.parent, true);
  }
  ExplicitSolveLists o;
  for (int32_t q : t.eliminationList) {
    bool nz = force[size_t(q)] != 0;
    for (int32_t e = t.colStart[size_t(q)]; !nz && e < t.colStart[size_t(q) + 1]; ++e) {
      const ColumnSource& cs = t.colSources[size_t(e)];
      nz = (cs.dof >= 3 && cs.dof < 6) ? anyBelow[size_t(cs.joint)] != 0 : pointBelow[size_t(cs.joint)] != 0;
    }
    if (nz) {
      o.list.push_back(q);
    }
  }
  if (o.list.empty()) {
    o.list = t.eliminationList; // nothing to solve for: keep the plain system (all steps are zero)
  }
  o.sorted = o.list;
  std::sort(o.sorted.begin(), o.sorted.end());
  return o;
}

bool tileStructureDense(const FusedTables& f, const std::vector<int32_t>& explicitList, int32_t GT) {
  const int32_t n = int32_t(f.solveList.size());
  return f.solveList != explicitList || n > 512 || GT > 0 || n == 0;
}

std::vector<uint8_t> buildRelatedness(const mmx_rig_desc* d, const FusedTables& f, const std::vector<std::pair<int32_t, int32_t>>& limitPairs) {
  const int32_t n = int32_t(f.solveList.size());
  const size_t J = size_t(d->num_joints);
  std::vector<uint8_t> reach(size_t(n) * J, 0); // joints in an ancestor relation with some source joint of column c
  for (int32_t c = 0; c < n; ++c) {
    uint8_t* rc = reach.data() + size_t(c) * J;
    for (int32_t e = f.srcStart[size_t(c)]; e < f.srcStart[size_t(c) + 1]; ++e) {
      const ColumnSource& cs = f.srcs[size_t(e)];
      for (int32_t k = cs.tin; k < cs.tout; ++k) {
        rc[size_t(f.dfsJoint[size_t(k)])] = 1;
      }
      for (int32_t a = cs.parent; a >= 0; a = d->parent[size_t(a)]) {
        rc[size_t(a)] = 1;
      }
    }
  }
  std::vector<uint8_t> related(size_t(n) * size_t(n), 0);
  for (int32_t row = 0; row < n; ++row) {
    for (int32_t col = 0; col < row; ++col) {
      const uint8_t* rc = reach.data() + size_t(col) * J;
      bool any = false;
      for (int32_t e = f.srcStart[size_t(row)]; !any && e < f.srcStart[size_t(row) + 1]; ++e) {
        any = rc[size_t(f.srcs[size_t(e)].joint)] != 0;
      }
      related[size_t(row) * size_t(n) + size_t(col)] = any ? 1 : 0;
    }
  }
  for (const auto& rcPair : limitPairs) {
    related[size_t(rcPair.first) * size_t(n) + size_t(rcPair.second)] = 1;
  }
  return related;
}

std::vector<uint32_t> packTileMasks(const TileMasks& m) {
  std::vector<uint32_t> masks(96, 0u);
  uint32_t base = 0;
  for (int i = 0; i < 32; ++i) {
    masks[size_t(i)] = m.rowMask[i];
    masks[size_t(32 + i)] = m.colMask[i];
    masks[size_t(64 + i)] = base; // first slot of block column i in the column-compact numbering
    base += uint32_t(__builtin_popcount(m.colMask[i]));
  }
  for (int k = 0; k < m.NB && k < 32; ++k) {
    for (int I = k; I < 32; ++I) {
      if (m.colMask[k] >> I & 1u) {
        masks.push_back(uint32_t(I) | uint32_t(k) << 8);
      }
    }
  }
  for (int32_t w : m.levelSteps) {
    masks.push_back(uint32_t(w));
  }
  return masks;
}

CompactRig buildCompactRig(const mmx_rig_desc* d, const LiveJoints& lj) {
  CompactRig o;
  const size_t nJc = size_t(lj.numLive);
  o.parent.resize(nJc);
  o.ptOuter.assign(1, 0);
  o.preRot.resize(4 * nJc);
  o.offset.resize(3 * nJc);
  for (int32_t c = 0; c < lj.numLive; ++c) {
    const int32_t j = lj.fullOf[size_t(c)];
    o.parent[size_t(c)] = d->parent[size_t(j)] < 0 ? d->parent[size_t(j)] : lj.compactOf[size_t(d->parent[size_t(j)])];
    std::copy_n(&d->pre_rotation[4 * size_t(j)], 4, &o.preRot[4 * size_t(c)]);
    std::copy_n(&d->translation_offset[3 * size_t(j)], 3, &o.offset[3 * size_t(c)]);
    for (int32_t dof = 0; dof < MMX_PARAMS_PER_JOINT; ++dof) {
      const size_t row = size_t(MMX_PARAMS_PER_JOINT) * size_t(j) + size_t(dof);
      o.ptInner.insert(o.ptInner.end(), d->pt_inner + d->pt_outer[row], d->pt_inner + d->pt_outer[row + 1]);
      o.ptValue.insert(o.ptValue.end(), d->pt_value + d->pt_outer[row], d->pt_value + d->pt_outer[row + 1]);
      o.ptOuter.push_back(int32_t(o.ptInner.size()));
      o.ptOffsets.push_back(d->pt_offsets[row]);
    }
  }
  return o;
}

CompactOrder buildCompactOrder(const HostTables& t, const FusedTables& f, const LiveJoints& lj) {
  CompactOrder o;
  const int32_t J = t.J, Jc = lj.numLive;
  int32_t maxLevel = 0;
  for (int32_t j : lj.fullOf) {
    maxLevel = std::max(maxLevel, t.level[size_t(j)]);
  }
  o.levelStart.assign(size_t(maxLevel) + 2, 0);
  for (int32_t j : lj.fullOf) {
    o.levelStart[size_t(t.level[size_t(j)]) + 1]++;
  }
  for (int32_t l = 0; l <= maxLevel; ++l) {
    o.levelStart[size_t(l) + 1] += o.levelStart[size_t(l)];
  }
  o.levelOrder.resize(size_t(Jc));
  std::vector<int32_t> cursor(o.levelStart.begin(), o.levelStart.end() - 1);
  for (int32_t c = 0; c < Jc; ++c) {
    o.levelOrder[size_t(cursor[size_t(t.level[size_t(lj.fullOf[size_t(c)])])]++)] = c;
  }
  o.posOf.assign(size_t(J), -1);
  std::vector<int32_t> liveBefore(size_t(J) + 1, 0); // live positions before full position k
  for (int32_t k = 0; k < J; ++k) { // full DFS positions, ascending
    const bool live = lj.live[size_t(f.dfsJoint[size_t(k)])] != 0;
    if (live) {
      o.posOf[size_t(k)] = liveBefore[size_t(k)];
    }
    liveBefore[size_t(k) + 1] = liveBefore[size_t(k)] + (live ? 1 : 0);
  }
  o.tin.resize(size_t(Jc));
  o.tout.resize(size_t(Jc));
  for (int32_t c = 0; c < Jc; ++c) {
    const int32_t j = lj.fullOf[size_t(c)];
    o.tin[size_t(c)] = liveBefore[size_t(t.tin[size_t(j)])];
    o.tout[size_t(c)] = liveBefore[size_t(t.tout[size_t(j)])];
  }
  return o;
}

LiveView buildLiveView(
    const mmx_rig_desc* d, const HostTables& t, const FusedTables& f, const ProblemTopology& p, const LiveJoints& lj,
    const std::vector<ColumnSource>& slots) {
  LiveView v;
  const int32_t J = t.J, Jc = lj.numLive, U = p.U();
  v.rig = buildCompactRig(d, lj);
  v.order = buildCompactOrder(t, f, lj);
  const std::vector<int32_t>&cTin = v.order.tin, &cTout = v.order.tout, &posOf = v.order.posOf;
  v.derived = deriveRigTables(Jc, d->num_params, v.rig.parent, v.rig.ptOuter, v.rig.ptInner, v.rig.ptValue, int32_t(v.order.levelStart.size()) - 1);
  v.joints = buildJointTables(p, lj.compactOf.data(), cTin, cTout);
  auto cj = [&](int32_t j) { return j < 0 ? j : lj.compactOf[size_t(j)]; };
  auto crow = [&](int32_t row) { return MMX_PARAMS_PER_JOINT * cj(row / MMX_PARAMS_PER_JOINT) + row % MMX_PARAMS_PER_JOINT; };
  std::vector<mmx_parameter_limit> lims(p.limits);
  for (mmx_parameter_limit& lm : lims) {
    if (lm.type == MMX_LIMIT_MINMAX_JOINT || lm.type == MMX_LIMIT_LINEAR_JOINT) {
      lm.index0 = crow(lm.index0);
    }
    if (lm.type == MMX_LIMIT_LINEAR_JOINT) {
      lm.index1 = crow(lm.index1);
    }
  }
  v.limits = std::move(lims);
  // ---- the one-launch solve's tables by DFS position, and the slots
  v.subSize.resize(size_t(Jc));
  v.dfsJoint.resize(size_t(Jc));
  v.posUnitStart.assign(size_t(Jc) + 1, U);
  for (int32_t c = 0; c < Jc; ++c) {
    v.subSize[size_t(cTin[size_t(c)])] = cTout[size_t(c)] - cTin[size_t(c)];
    v.dfsJoint[size_t(cTin[size_t(c)])] = c;
  }
  for (int32_t k = 0; k < J; ++k) { // (a dead position carries no unit: the live rows of the CSR are the whole of it)
    if (posOf[size_t(k)] >= 0) {
      v.posUnitStart[size_t(posOf[size_t(k)])] = f.posUnitStart[size_t(k)];
      if (f.posUnitStart[size_t(k) + 1] > f.posUnitStart[size_t(k)]) {
        v.loadedPos.push_back(posOf[size_t(k)]);
      }
    }
  }
  v.slots = slots;
  for (ColumnSource& cs : v.slots) {
    if (cs.tin == cs.tout || !lj.live[size_t(cs.joint)]) { // a pad slot (weight 0, empty interval): any live joint will do
      cs = ColumnSource{0, cs.dof, 0, 0, -1, cs.weight};
      continue;
    }
    const int32_t c = lj.compactOf[size_t(cs.joint)];
    cs.joint = c;
    cs.parent = cj(cs.parent);
    cs.tin = cTin[size_t(c)];
    cs.tout = cTout[size_t(c)];
  }
  return v;
}

} // namespace mmx
