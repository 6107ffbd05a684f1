// The problem-table builders of momentum_amd/csrc/mmx_host_tables.hpp against brute-force restatements written here: every
// table is checked against an enumeration over joints, parents and transform rows, never against a second call of the code
// under test.  Stand-alone: links mmx_host_tables.cpp only, needs no GPU (tests/test_problem_tables_host.py builds it with
// the address and undefined-behaviour sanitizers).
#include "../../momentum_amd/csrc/mmx_host_tables.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>

namespace {

using mmx::ColumnSource;
using Ints = std::vector<int32_t>;

const char* g_case = "";
#define CHECK(...)                                                                     \
  do {                                                                                 \
    if (!(__VA_ARGS__)) {                                                              \
      std::printf("FAILED [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #__VA_ARGS__); \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

struct Triplet {
  int32_t row, param;
  float value;
};

struct Rig {
  int32_t J = 0, P = 0;
  Ints parent, ptOuter, ptInner;
  std::vector<float> preRot, offset, ptValue, ptOffsets;
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

// parents + transform entries (any order); one float pattern per joint so that a copied row is recognisable
Rig makeRig(const Ints& parent, std::vector<Triplet> trip, int32_t P) {
  Rig r;
  r.J = int32_t(parent.size());
  r.P = P;
  r.parent = parent;
  std::stable_sort(trip.begin(), trip.end(), [](const Triplet& a, const Triplet& b) { return a.row < b.row; });
  r.ptOuter.assign(size_t(7 * r.J) + 1, 0);
  for (const Triplet& t : trip) {
    r.ptOuter[size_t(t.row) + 1]++;
    r.ptInner.push_back(t.param);
    r.ptValue.push_back(t.value);
  }
  for (int32_t row = 0; row < 7 * r.J; ++row) {
    r.ptOuter[size_t(row) + 1] += r.ptOuter[size_t(row)];
    r.ptOffsets.push_back(0.25f * float(row));
  }
  for (int32_t j = 0; j < r.J; ++j) {
    for (int k = 0; k < 4; ++k) {
      r.preRot.push_back(float(10 * j + k));
    }
    for (int k = 0; k < 3; ++k) {
      r.offset.push_back(float(100 * j + k));
    }
  }
  return r;
}

// one rotation parameter per joint (parameter j = row 7 j + 3), then the given shared entries
Rig treeRig(const Ints& parent, const std::vector<Triplet>& shared = {}, int32_t extraParams = 0) {
  std::vector<Triplet> trip;
  for (int32_t j = 0; j < int32_t(parent.size()); ++j) {
    trip.push_back(Triplet{7 * j + 3, j, 1.f + 0.5f * float(j)});
  }
  trip.insert(trip.end(), shared.begin(), shared.end());
  return makeRig(parent, trip, int32_t(parent.size()) + extraParams);
}

bool ancestorOrSelf(const Ints& parent, int32_t a, int32_t j) { // walks j's chain upwards
  for (; j >= 0; j = parent[size_t(j)]) {
    if (j == a) {
      return true;
    }
  }
  return false;
}
bool inRelation(const Ints& parent, int32_t a, int32_t b) {
  return ancestorOrSelf(parent, a, b) || ancestorOrSelf(parent, b, a);
}

bool fixedAxis(int32_t type) {
  return type == MMX_JC_FIXED_AXIS_DIFF || type == MMX_JC_FIXED_AXIS_COS || type == MMX_JC_FIXED_AXIS_ANGLE;
}

// every constraint vector of the problem: (joint, is it a point)
std::vector<std::pair<int32_t, bool>> constraintVectors(const mmx::ProblemTopology& p) {
  std::vector<std::pair<int32_t, bool>> v;
  for (int32_t j : p.posParent) {
    v.push_back({j, true});
  }
  for (int32_t j : p.oriParent) {
    v.push_back({j, false});
  }
  if (p.instPos) {
    for (int32_t j : p.unionPos) {
      v.push_back({j, true});
    }
  }
  if (p.instOri) {
    for (int32_t j : p.unionOri) {
      v.push_back({j, false});
    }
  }
  for (const auto& b : p.blocks) {
    for (int32_t j : b.parent) {
      v.push_back({j, !fixedAxis(b.type)});
    }
    for (int32_t j : b.parentB) {
      v.push_back({j, true});
    }
  }
  for (const mmx_ellipsoid_limit& e : p.ellipsoids) {
    v.push_back({e.parent, true});
  }
  return v;
}

// the model parameters of a limit, restated: the parameters themselves, or the columns of the limited transform rows
std::set<int32_t> limitParams(const Rig& r, const mmx_parameter_limit& lm) {
  std::set<int32_t> s;
  auto row = [&](int32_t rw) {
    for (int32_t k = r.ptOuter[size_t(rw)]; k < r.ptOuter[size_t(rw) + 1]; ++k) {
      s.insert(r.ptInner[size_t(k)]);
    }
  };
  if (lm.type == MMX_LIMIT_MINMAX) {
    s.insert(lm.index0);
  } else if (lm.type == MMX_LIMIT_LINEAR || lm.type == MMX_LIMIT_HALFPLANE) {
    s.insert(lm.index0), s.insert(lm.index1);
  } else if (lm.type == MMX_LIMIT_MINMAX_JOINT) {
    row(lm.index0);
  } else if (lm.type == MMX_LIMIT_LINEAR_JOINT) {
    row(lm.index0), row(lm.index1);
  }
  return s;
}

struct Src {
  int32_t joint, dof;
  float weight;
};

// tile-region offset of entry (row, col), restated: tiles row-major over the lower triangle, 256 floats each; inside a tile
// the row, then the column's group of four XOR the row's group, then the column within the group
int32_t entryOffset(int32_t row, int32_t col) {
  const int32_t tile = (row / 16) * (row / 16 + 1) / 2 + col / 16;
  const int32_t r = row % 16, c = col % 16;
  return tile * 256 + r * 16 + 4 * ((c / 4) ^ (r / 4)) + c % 4;
}

bool sameSource(const ColumnSource& s, const Src& b, const Rig& r, const mmx::HostTables& t) {
  return s.joint == b.joint && s.dof == b.dof && s.weight == b.weight && s.parent == r.parent[size_t(b.joint)] && s.tin == t.tin[size_t(b.joint)] &&
      s.tout == t.tout[size_t(b.joint)];
}

void checkCase(const char* name, const Rig& rig, const mmx::ProblemTopology& topo, const std::vector<uint8_t>& enabledIn = {}) {
  g_case = name;
  const mmx_rig_desc d = rig.desc();
  const int32_t J = rig.J, P = rig.P, U = topo.U();
  std::string err;
  mmx::HostTables t;
  CHECK(mmx::buildHostTables(&d, enabledIn.empty() ? nullptr : enabledIn.data(), t, err) == MMX_OK);
  std::vector<uint8_t> enabled(size_t(P), 1);
  if (!enabledIn.empty()) {
    enabled = enabledIn;
  }

  // ---- brute-force facts
  const auto vectors = constraintVectors(topo);
  std::vector<uint8_t> anyBelow(size_t(J), 0), pointBelow(size_t(J), 0);
  for (int32_t a = 0; a < J; ++a) {
    for (const auto& v : vectors) {
      if (ancestorOrSelf(rig.parent, a, v.first)) {
        anyBelow[size_t(a)] = 1;
        pointBelow[size_t(a)] |= v.second ? 1 : 0;
      }
    }
  }
  auto movable = [&](const Src& s) { return (s.dof >= 3 && s.dof < 6) ? anyBelow[size_t(s.joint)] != 0 : pointBelow[size_t(s.joint)] != 0; };
  const size_t nP = size_t(P);
  std::vector<std::vector<Src>> sources(nP), moving(nP); // enabled columns, in row order; the movable ones of them
  for (int32_t row = 0; row < 7 * J; ++row) {
    for (int32_t k = rig.ptOuter[size_t(row)]; k < rig.ptOuter[size_t(row) + 1]; ++k) {
      const int32_t p = rig.ptInner[size_t(k)];
      if (enabled[size_t(p)]) {
        const Src s{row / 7, row % 7, rig.ptValue[size_t(k)]};
        sources[size_t(p)].push_back(s);
        if (movable(s)) {
          moving[size_t(p)].push_back(s);
        }
      }
    }
  }
  std::vector<uint8_t> forced(size_t(P), topo.hasModel ? 1 : 0);
  for (const mmx_parameter_limit& lm : topo.limits) {
    for (int32_t p : limitParams(rig, lm)) {
      forced[size_t(p)] = 1;
    }
  }

  // ---- limitParameters, structure lists
  for (const mmx_parameter_limit& lm : topo.limits) {
    const Ints got = mmx::limitParameters(&d, lm);
    const std::set<int32_t> want = limitParams(rig, lm);
    CHECK(std::set<int32_t>(got.begin(), got.end()) == want && got.size() == want.size());
  }
  const mmx::StructureLists sl = mmx::buildStructureLists(&d, topo);
  CHECK(sl.force == forced);
  {
    std::multiset<int32_t> wantPos, wantOri; // beyond posParent / oriParent, which buildFusedTables gets as they are
    for (size_t i = size_t(topo.Kp + topo.Ko); i < vectors.size(); ++i) {
      (vectors[i].second ? wantPos : wantOri).insert(vectors[i].first);
    }
    CHECK(std::multiset<int32_t>(sl.structPos.begin(), sl.structPos.end()) == wantPos);
    CHECK(std::multiset<int32_t>(sl.structOri.begin(), sl.structOri.end()) == wantOri);
  }
  mmx::FusedTables f;
  CHECK(mmx::buildProblemFusedTables(&d, t, topo, sl, f, err) == MMX_OK);
  const int32_t n = int32_t(f.solveList.size());
  for (int32_t p = 0; p < P; ++p) { // (the fused solve list itself: the forced and the structurally non-zero, in elimination order)
    const bool in = std::find(f.solveList.begin(), f.solveList.end(), p) != f.solveList.end();
    CHECK(in == (enabled[size_t(p)] && (forced[size_t(p)] || !moving[size_t(p)].empty())));
  }

  // ---- joint tables of the full rig
  const mmx::JointTables jt = mmx::buildJointTables(topo, nullptr, t.tin, t.tout);
  Ints unitJointWant;
  {
    for (int32_t j : topo.posParent) {
      unitJointWant.push_back(j);
    }
    for (int32_t j : topo.oriParent) {
      unitJointWant.insert(unitJointWant.end(), 3, j);
    }
    CHECK(jt.unitJoint.size() == size_t(std::max(U, 1)) && jt.unitTin.size() == jt.unitJoint.size());
    for (int32_t u = 0; u < U; ++u) {
      CHECK(jt.unitJoint[size_t(u)] == unitJointWant[size_t(u)] && jt.unitTin[size_t(u)] == t.tin[size_t(unitJointWant[size_t(u)])]);
    }
    Ints gj, gb, gj2;
    for (size_t b = 0; b < topo.blocks.size(); ++b) {
      for (size_t c = 0; c < topo.blocks[b].parent.size(); ++c) {
        gj.push_back(topo.blocks[b].parent[c]);
        gb.push_back(int32_t(b));
        gj2.push_back(topo.blocks[b].parentB.empty() ? -1 : topo.blocks[b].parentB[c]);
      }
    }
    const size_t G = gj.size();
    CHECK(jt.genBlock == gb && jt.genJoint.size() == 2 * G && jt.genTin.size() == 2 * G);
    for (size_t g = 0; g < G; ++g) {
      CHECK(jt.genJoint[g] == gj[g] && jt.genTin[g] == t.tin[size_t(gj[g])]);
      CHECK(jt.genJoint[G + g] == gj2[g] && jt.genTin[G + g] == (gj2[g] < 0 ? -1 : t.tin[size_t(gj2[g])]));
    }
    CHECK(jt.ellTinParent.size() == topo.ellipsoids.size() && jt.ellTinStop.size() == topo.ellipsoids.size());
    for (size_t i = 0; i < topo.ellipsoids.size(); ++i) {
      const mmx_ellipsoid_limit& e = topo.ellipsoids[i];
      CHECK(jt.ellParent[i] == e.parent && jt.ellEllipsoidParent[i] == e.ellipsoid_parent && jt.ellTinParent[i] == t.tin[size_t(e.parent)]);
      CHECK(jt.ellTinStop[i] == (ancestorOrSelf(rig.parent, e.ellipsoid_parent, e.parent) ? t.tin[size_t(e.ellipsoid_parent)] : -1));
    }
  }

  // ---- column program
  {
    const mmx::ColumnProgram cp = mmx::buildColumnProgram(t, f);
    std::vector<int> seen(size_t(P), 0);
    std::vector<std::tuple<int32_t, int32_t, int32_t>> real; // (joint, dof, column) of the single-source rotation columns
    for (int32_t p = 0; p < P; ++p) {
      const bool zero = !enabled[size_t(p)] || moving[size_t(p)].empty();
      CHECK((std::find(cp.zero.begin(), cp.zero.end(), p) != cp.zero.end()) == zero);
      seen[size_t(p)] += int(std::count(cp.zero.begin(), cp.zero.end(), p)) + int(std::count(cp.multi.begin(), cp.multi.end(), p));
      if (!zero && sources[size_t(p)].size() == 1 && sources[size_t(p)][0].dof >= 3 && sources[size_t(p)][0].dof < 6) {
        real.push_back({sources[size_t(p)][0].joint, sources[size_t(p)][0].dof, p});
      }
    }
    std::sort(real.begin(), real.end());
    CHECK(cp.recs.size() % 4 == 0 && cp.recs.size() >= real.size() && cp.recs.size() < real.size() + 4 && (real.empty() == cp.recs.empty()));
    for (size_t i = 0; i < cp.recs.size(); ++i) {
      const mmx::JacRec& rc = cp.recs[i];
      if (i < real.size()) {
        CHECK(std::make_tuple(rc.joint, rc.dof, rc.col) == real[i]);
        CHECK(sameSource(ColumnSource{rc.joint, rc.dof, rc.tin, rc.tout, rc.parent, rc.weight}, sources[size_t(rc.col)][0], rig, t));
        seen[size_t(rc.col)]++;
      } else {
        CHECK(std::memcmp(&rc, &cp.recs[real.size() - 1], sizeof(rc)) == 0);
      }
    }
    for (int32_t p = 0; p < P; ++p) {
      CHECK(seen[size_t(p)] == 1);
    }
  }

  // ---- slots
  const int32_t slotBlocks = std::max((n + 15) / 16, 1);
  const mmx::SlotTables st = mmx::buildSlotTables(f, slotBlocks);
  const size_t nCols = size_t(n);
  std::vector<Ints> slotsOfColumn(nCols); // the slots of column c's sources, primary first
  {
    CHECK(st.slotBase == 16 * slotBlocks && st.slots.size() % 4 == 0 && st.xStart.size() == size_t(st.slotBase) + 1);
    std::vector<uint8_t> used(st.slots.size(), 0);
    int32_t extras = 0;
    for (int32_t c = 0; c < n; ++c) {
      const std::vector<Src>& m = moving[size_t(f.solveList[size_t(c)])];
      CHECK(st.xStart[size_t(c)] == extras);
      for (size_t i = 0; i < m.size(); ++i) {
        const int32_t slot = i == 0 ? c : st.slotBase + extras++;
        CHECK(size_t(slot) < st.slots.size() && sameSource(st.slots[size_t(slot)], m[i], rig, t));
        used[size_t(slot)] = 1;
        slotsOfColumn[size_t(c)].push_back(slot);
      }
    }
    for (int32_t c = n; c <= st.slotBase; ++c) {
      CHECK(st.xStart[size_t(c)] == extras);
    }
    CHECK(st.slots.size() >= size_t(st.slotBase + extras) && st.slots.size() < size_t(st.slotBase + extras) + 4);
    for (size_t s = 0; s < st.slots.size(); ++s) {
      if (!used[s]) {
        CHECK(st.slots[s].weight == 0.f && st.slots[s].tin == st.slots[s].tout);
      }
    }
    Ints loaded;
    for (int32_t k = 0; k < J; ++k) {
      bool any = false;
      for (int32_t u = 0; u < U; ++u) {
        any = any || t.tin[size_t(unitJointWant[size_t(u)])] == k;
      }
      if (any) {
        loaded.push_back(k);
      }
    }
    CHECK(st.loadedPos == loaded);
  }

  // ---- term records
  {
    using Term = std::tuple<int32_t, int32_t, int32_t>; // (entry's offset, deep slot, ancestor slot)
    std::vector<Term> want;
    std::map<int32_t, size_t> termsOfEntry;
    for (int32_t row = 0; row < n; ++row) {
      for (int32_t col = 0; col <= row; ++col) {
        const std::vector<Src>&mr = moving[size_t(f.solveList[size_t(row)])], &mc = moving[size_t(f.solveList[size_t(col)])];
        for (size_t a = 0; a < mr.size(); ++a) {
          for (size_t b = 0; b < mc.size(); ++b) {
            if ((a == 0 && b == 0) || !inRelation(rig.parent, mr[a].joint, mc[b].joint)) {
              continue;
            }
            const bool rowIsDeep = ancestorOrSelf(rig.parent, mc[b].joint, mr[a].joint);
            const int32_t sr = slotsOfColumn[size_t(row)][a], sc = slotsOfColumn[size_t(col)][b];
            want.push_back({entryOffset(row, col), rowIsDeep ? sr : sc, rowIsDeep ? sc : sr});
            termsOfEntry[entryOffset(row, col)]++;
          }
        }
      }
    }
    std::sort(want.begin(), want.end());
    size_t cellsWant = 0;
    for (const auto& kv : termsOfEntry) {
      cellsWant += (kv.second + 7) / 8 - 1;
    }
    mmx::TermRuns runs;
    CHECK(mmx::buildTermRuns(f, st, J, runs, err) == MMX_OK);
    CHECK(size_t(runs.numCells) == cellsWant && runs.comb.size() % 3 == 0);
    std::map<int32_t, int32_t> entryOfCell;
    for (size_t i = 0; i < runs.comb.size(); i += 3) {
      CHECK(termsOfEntry.count(runs.comb[i]) == 1 && size_t(runs.comb[i + 2]) == (termsOfEntry[runs.comb[i]] + 7) / 8 - 1);
      for (int32_t c = 0; c < runs.comb[i + 2]; ++c) {
        CHECK(entryOfCell.emplace(runs.comb[i + 1] + c, runs.comb[i]).second);
      }
    }
    CHECK(entryOfCell.size() == cellsWant && (cellsWant == 0 || (entryOfCell.begin()->first == 0 && entryOfCell.rbegin()->first == int32_t(cellsWant) - 1)));
    for (int threads : {256, 1024}) {
      std::vector<uint32_t> words;
      const size_t rounds = mmx::dealTermRuns(runs, threads, words);
      CHECK(rounds % 8 == 0 && words.size() == std::max<size_t>(rounds, 8) * size_t(threads) * 4);
      std::vector<Term> got;
      std::set<int32_t> cellsSeen, directSeen;
      size_t most = 0, least = ~size_t(0);
      for (int th = 0; th < threads; ++th) {
        size_t count = 0, inRun = 0;
        uint32_t runDest = 0;
        bool ended = false;
        for (size_t k = 0; k < words.size() / (size_t(threads) * 4); ++k) {
          const uint32_t* w = &words[(k * size_t(threads) + size_t(th)) * 4];
          if (w[0] == 0) { // behind a thread's last record: zeros to the end
            ended = true;
            CHECK(w[1] == 0 && w[2] == 0 && w[3] == 0 && inRun == 0);
            continue;
          }
          CHECK(!ended && (w[0] >> 26 & 1u) && w[3] == 0);
          const float one = 1.f;
          CHECK(std::memcmp(&w[2], &one, 4) == 0);
          CHECK(((w[0] >> 24 & 1u) != 0) == (inRun == 0)); // the first flag on a run's first record only
          if (inRun == 0) {
            runDest = w[1];
            const bool cell = (w[1] >> 30 & 1u) != 0;
            CHECK((cell ? cellsSeen.insert(int32_t(w[1] & 0x3fffffffu)) : directSeen.insert(int32_t(w[1]))).second); // one run per cell / entry
          }
          CHECK(w[1] == runDest);
          ++inRun, ++count;
          CHECK(inRun <= 8);
          const bool cell = (w[1] >> 30 & 1u) != 0;
          const int32_t cellIndex = int32_t(w[1] & 0x3fffffffu);
          CHECK(!cell || entryOfCell.count(cellIndex) == 1);
          got.push_back({cell ? entryOfCell[cellIndex] : int32_t(w[1]), int32_t(w[0] & 0xfffu), int32_t(w[0] >> 12 & 0xfffu)});
          if (w[0] >> 25 & 1u) {
            inRun = 0;
          }
        }
        CHECK(inRun == 0); // the last flag closed the thread's last run
        most = std::max(most, count), least = std::min(least, count);
      }
      std::sort(got.begin(), got.end());
      CHECK(got == want); // (so the 256- and the 1024-thread deal decode to the same multiset)
      CHECK(cellsSeen.size() == cellsWant && directSeen.size() == termsOfEntry.size());
      CHECK(most - least <= 8);
    }
  }

  // ---- limit tables, relatedness, tile masks
  mmx::LimitTables lt = mmx::buildLimitTables(&d, topo.limits, f.solveList);
  {
    auto columnOf = [&](int32_t p) {
      const auto it = std::find(f.solveList.begin(), f.solveList.end(), p);
      return it == f.solveList.end() ? -1 : int32_t(it - f.solveList.begin());
    };
    std::map<std::pair<int32_t, int32_t>, Ints> coupled; // (row, col), row > col -> the limits that couple them, ascending
    std::vector<Ints> limitsOf(size_t(std::max(n, 1)));
    for (size_t l = 0; l < topo.limits.size(); ++l) {
      std::set<int32_t> cols;
      for (int32_t p : limitParams(rig, topo.limits[l])) {
        if (columnOf(p) >= 0) {
          cols.insert(columnOf(p));
        }
      }
      for (int32_t a : cols) {
        limitsOf[size_t(a)].push_back(int32_t(l));
        for (int32_t b : cols) {
          if (a > b) {
            coupled[{a, b}].push_back(int32_t(l));
          }
        }
      }
    }
    CHECK(lt.limStart.size() == size_t(n) + 1 && lt.limStart[0] == 0);
    for (int32_t c = 0; c < n; ++c) {
      CHECK(Ints(lt.limOf.begin() + lt.limStart[size_t(c)], lt.limOf.begin() + lt.limStart[size_t(c) + 1]) == limitsOf[size_t(c)]);
    }
    CHECK(size_t(lt.limStart.back()) == lt.limOf.size());
    CHECK(std::set<std::pair<int32_t, int32_t>>(lt.limitPairs.begin(), lt.limitPairs.end()).size() == coupled.size() && lt.limitPairs.size() == coupled.size());
    CHECK(lt.pairDest.size() == coupled.size() && lt.pairStart.size() == coupled.size() + 1 && lt.pairCols.size() == 2 * coupled.size());
    CHECK(std::is_sorted(lt.pairDest.begin(), lt.pairDest.end()));
    for (size_t i = 0; i < lt.limitPairs.size(); ++i) {
      const auto rc = lt.limitPairs[i];
      CHECK(coupled.count(rc) == 1 && lt.pairDest[i] == entryOffset(rc.first, rc.second) && lt.pairCols[2 * i] == rc.first && lt.pairCols[2 * i + 1] == rc.second);
      CHECK(Ints(lt.pairLim.begin() + lt.pairStart[i], lt.pairLim.begin() + lt.pairStart[i + 1]) == coupled[rc]);
    }
    const std::vector<uint8_t> related = mmx::buildRelatedness(&d, f, lt.limitPairs);
    CHECK(related.size() == size_t(n) * size_t(n));
    for (int32_t row = 0; row < n; ++row) {
      for (int32_t col = 0; col < row; ++col) {
        bool want = coupled.count({row, col}) == 1;
        for (const Src& a : moving[size_t(f.solveList[size_t(row)])]) {
          for (const Src& b : moving[size_t(f.solveList[size_t(col)])]) {
            want = want || inRelation(rig.parent, a.joint, b.joint);
          }
        }
        CHECK((related[size_t(row) * size_t(n) + size_t(col)] != 0) == want);
      }
    }
    // the packed mask array around eliminationTileMasks
    if (n > 0) {
      const mmx::TileMasks tm = mmx::eliminationTileMasks(n, related, false);
      const std::vector<uint32_t> packed = mmx::packTileMasks(tm);
      CHECK(packed.size() == 96 + tm.tiles.size() + tm.levelSteps.size());
      size_t slot = 96;
      for (int k = 0; k < 32; ++k) {
        CHECK(packed[size_t(k)] == tm.rowMask[k] && packed[32 + size_t(k)] == tm.colMask[k] && packed[64 + size_t(k)] == slot - 96);
        for (int I = 0; I < 32; ++I) {
          if (tm.colMask[k] >> I & 1u) {
            CHECK(packed[slot++] == (uint32_t(I) | uint32_t(k) << 8));
          }
        }
      }
      CHECK(slot == 96 + tm.tiles.size());
      for (size_t i = 0; i < tm.levelSteps.size(); ++i) {
        CHECK(packed[slot + i] == uint32_t(tm.levelSteps[i]));
      }
    }
  }

  // ---- the explicit-Jacobian solve list and the double solve's
  const mmx::ExplicitSolveLists xl = mmx::buildExplicitSolveLists(&d, t, topo, sl.force);
  {
    Ints want;
    for (int32_t p : t.eliminationList) { // a sub-sequence of the elimination order
      if (forced[size_t(p)] || !moving[size_t(p)].empty()) {
        want.push_back(p);
      }
    }
    if (want.empty()) {
      want = t.eliminationList;
    }
    CHECK(xl.list == want);
    std::sort(want.begin(), want.end());
    CHECK(xl.sorted == want);
    const int32_t GT = int32_t(jt.genBlock.size() + topo.ellipsoids.size());
    CHECK(mmx::tileStructureDense(f, xl.list, GT) == (GT > 0 || n == 0 || n > 512 || xl.list != f.solveList));
  }

  // ---- the live-joint view against the tables of the compacted rig, built from scratch
  if (topo.instPos || topo.instOri) {
    return; // (no view with per-instance parents)
  }
  std::vector<uint8_t> live(size_t(J), 0);
  {
    Ints ref;
    for (const auto& v : vectors) {
      ref.push_back(v.first);
    }
    for (const mmx_ellipsoid_limit& e : topo.ellipsoids) {
      ref.push_back(e.ellipsoid_parent);
    }
    for (const mmx_parameter_limit& lm : topo.limits) {
      if (lm.type == MMX_LIMIT_MINMAX_JOINT || lm.type == MMX_LIMIT_LINEAR_JOINT) {
        ref.push_back(lm.index0 / 7);
      }
      if (lm.type == MMX_LIMIT_LINEAR_JOINT) {
        ref.push_back(lm.index1 / 7);
      }
    }
    for (int32_t a = 0; a < J; ++a) {
      for (int32_t j : ref) {
        live[size_t(a)] |= ancestorOrSelf(rig.parent, a, j) ? 1 : 0;
      }
    }
    Ints got = mmx::referencedJoints(topo);
    std::sort(got.begin(), got.end());
    std::sort(ref.begin(), ref.end());
    CHECK(got == ref);
    mmx::LiveJoints lj;
    mmx::buildLiveJoints(rig.parent.data(), J, got.data(), int32_t(got.size()), lj);
    CHECK(lj.live == live);
    const mmx::LiveView lv = mmx::buildLiveView(&d, t, f, topo, lj, st.slots);

    auto cj = [&](int32_t j) { return j < 0 ? j : lj.compactOf[size_t(j)]; };
    Ints cParent;
    std::vector<Triplet> cTrip;
    for (int32_t j : lj.fullOf) {
      cParent.push_back(cj(rig.parent[size_t(j)]));
      for (int32_t row = 7 * j; row < 7 * j + 7; ++row) {
        for (int32_t k = rig.ptOuter[size_t(row)]; k < rig.ptOuter[size_t(row) + 1]; ++k) {
          cTrip.push_back(Triplet{7 * cj(j) + row % 7, rig.ptInner[size_t(k)], rig.ptValue[size_t(k)]});
        }
      }
    }
    const Rig cr = makeRig(cParent, cTrip, P);
    const int32_t Jc = cr.J;
    const mmx_rig_desc cd = cr.desc();
    mmx::ProblemTopology ctopo = topo;
    for (Ints* list : {&ctopo.posParent, &ctopo.oriParent}) {
      for (int32_t& j : *list) {
        j = cj(j);
      }
    }
    for (auto& b : ctopo.blocks) {
      for (Ints* list : {&b.parent, &b.parentB}) {
        for (int32_t& j : *list) {
          j = cj(j);
        }
      }
    }
    for (mmx_ellipsoid_limit& e : ctopo.ellipsoids) {
      e.parent = cj(e.parent), e.ellipsoid_parent = cj(e.ellipsoid_parent);
    }
    for (mmx_parameter_limit& lm : ctopo.limits) {
      if (lm.type == MMX_LIMIT_MINMAX_JOINT || lm.type == MMX_LIMIT_LINEAR_JOINT) {
        lm.index0 = 7 * cj(lm.index0 / 7) + lm.index0 % 7;
      }
      if (lm.type == MMX_LIMIT_LINEAR_JOINT) {
        lm.index1 = 7 * cj(lm.index1 / 7) + lm.index1 % 7;
      }
    }
    mmx::HostTables ct;
    mmx::FusedTables cf;
    CHECK(mmx::buildHostTables(&cd, enabledIn.empty() ? nullptr : enabledIn.data(), ct, err) == MMX_OK);
    Ints cStructPos, cStructOri;
    for (size_t i = size_t(topo.Kp + topo.Ko); i < vectors.size(); ++i) {
      (vectors[i].second ? cStructPos : cStructOri).push_back(cj(vectors[i].first));
    }
    CHECK(
        mmx::buildFusedTables(
            &cd, ct, ctopo.Kp, ctopo.posParent.data(), ctopo.Ko, ctopo.oriParent.data(), forced.data(), cStructPos.empty() ? nullptr : &cStructPos,
            cStructOri.empty() ? nullptr : &cStructOri, cf, err) == MMX_OK);
    // the compact rig, row by row
    CHECK(lv.rig.parent == cr.parent && lv.rig.ptOuter == cr.ptOuter && lv.rig.ptInner == cr.ptInner && lv.rig.ptValue == cr.ptValue);
    for (int32_t c = 0; c < Jc; ++c) {
      const size_t j = size_t(lj.fullOf[size_t(c)]);
      CHECK(std::equal(&rig.preRot[4 * j], &rig.preRot[4 * j] + 4, &lv.rig.preRot[4 * size_t(c)]));
      CHECK(std::equal(&rig.offset[3 * j], &rig.offset[3 * j] + 3, &lv.rig.offset[3 * size_t(c)]));
      CHECK(std::equal(&rig.ptOffsets[7 * j], &rig.ptOffsets[7 * j] + 7, &lv.rig.ptOffsets[7 * size_t(c)]));
    }
    CHECK(lv.rig.preRot.size() == 4 * size_t(Jc) && lv.rig.offset.size() == 3 * size_t(Jc) && lv.rig.ptOffsets.size() == 7 * size_t(Jc));
    // levels, intervals, positions
    CHECK(lv.order.levelStart == ct.levelStart && lv.order.levelOrder == ct.levelOrder);
    CHECK(lv.order.tin == ct.tin && lv.order.tout == ct.tout);
    CHECK(lv.subSize == cf.subSize && lv.dfsJoint == cf.dfsJoint);
    {
      Ints loaded;
      for (int32_t k = 0; k < Jc; ++k) {
        if (cf.posUnitStart[size_t(k) + 1] > cf.posUnitStart[size_t(k)]) {
          loaded.push_back(k);
        }
      }
      CHECK(lv.loadedPos == loaded);
    }
    // the pointer-jumping and transform-row tables of the compact rig, restated
    {
      const mmx::RigDerived& rd = lv.derived;
      int32_t rounds = 0;
      while ((1 << rounds) < int32_t(ct.levelStart.size()) - 1) {
        ++rounds;
      }
      CHECK(rd.jumpRounds == rounds && rd.jumpParent.size() == size_t(Jc));
      for (int32_t c = 0; c < Jc; ++c) {
        CHECK(rd.jumpParent[size_t(c)] == (cr.parent[size_t(c)] + 1) * 65537);
      }
      bool fits = true;
      for (int32_t row = 0; row < 7 * Jc; ++row) {
        fits = fits && cr.ptOuter[size_t(row) + 1] - cr.ptOuter[size_t(row)] <= 2;
      }
      CHECK(rd.ellOk == fits);
      size_t rec = 0;
      for (int32_t row = 0; row < 7 * Jc; ++row) {
        const int32_t k0 = cr.ptOuter[size_t(row)], cnt = cr.ptOuter[size_t(row) + 1] - k0;
        for (int s = 0; fits && s < 2; ++s) {
          int32_t bits = 0;
          if (s < cnt) {
            std::memcpy(&bits, &cr.ptValue[size_t(k0 + s)], 4);
          }
          CHECK(rd.ell[4 * size_t(row) + 2 * size_t(s)] == (s < cnt ? cr.ptInner[size_t(k0 + s)] : -1) && rd.ell[4 * size_t(row) + 2 * size_t(s) + 1] == bits);
        }
        if (cnt > 0) {
          int32_t next = row + 1, bits = 0;
          while (next < 7 * Jc && cr.ptOuter[size_t(next) + 1] == cr.ptOuter[size_t(next)]) {
            ++next;
          }
          std::memcpy(&bits, &cr.ptValue[size_t(k0)], 4);
          CHECK(rec + 4 <= rd.rowRec.size() && rd.rowRec[rec] == (row | (next - row) << 16) && rd.rowRec[rec + 1] == (cr.ptInner[size_t(k0)] | cnt << 16));
          CHECK(rd.rowRec[rec + 2] == bits && rd.rowRec[rec + 3] == k0);
          rec += 4;
        }
      }
      CHECK(rec == rd.rowRec.size());
    }
    // joint-indexed tables
    for (int32_t u = 0; u < U; ++u) {
      CHECK(lv.joints.unitJoint[size_t(u)] == cf.unitJoint[size_t(u)] && lv.joints.unitTin[size_t(u)] == ct.tin[size_t(cf.unitJoint[size_t(u)])]);
    }
    const size_t G = jt.genBlock.size();
    CHECK(lv.joints.genJoint.size() == 2 * G && lv.joints.genTin.size() == 2 * G);
    for (size_t g = 0; g < 2 * G; ++g) {
      const int32_t c = cj(jt.genJoint[g]);
      CHECK(lv.joints.genJoint[g] == c && lv.joints.genTin[g] == (c < 0 ? -1 : ct.tin[size_t(c)]));
    }
    for (size_t i = 0; i < topo.ellipsoids.size(); ++i) {
      const int32_t pj = ctopo.ellipsoids[i].parent, ep = ctopo.ellipsoids[i].ellipsoid_parent;
      CHECK(lv.joints.ellParent[i] == pj && lv.joints.ellEllipsoidParent[i] == ep && lv.joints.ellTinParent[i] == ct.tin[size_t(pj)]);
      CHECK(lv.joints.ellTinStop[i] == (ancestorOrSelf(cr.parent, ep, pj) ? ct.tin[size_t(ep)] : -1));
    }
    CHECK(lv.limits.size() == ctopo.limits.size());
    for (size_t l = 0; l < lv.limits.size(); ++l) {
      CHECK(std::memcmp(&lv.limits[l], &ctopo.limits[l], sizeof(mmx_parameter_limit)) == 0);
    }
    // posUnitStart: the full rig's value at every live position (its indices into posUnits are not renumbered), U at the end
    CHECK(lv.posUnitStart.size() == size_t(Jc) + 1 && lv.posUnitStart.back() == U);
    for (int32_t j : lj.fullOf) {
      CHECK(lv.posUnitStart[size_t(ct.tin[size_t(cj(j))])] == f.posUnitStart[size_t(t.tin[size_t(j)])]);
    }
    // slots
    CHECK(lv.slots.size() == st.slots.size());
    for (size_t s = 0; s < st.slots.size(); ++s) {
      const ColumnSource &full = st.slots[s], &got = lv.slots[s];
      CHECK(got.dof == full.dof && got.weight == full.weight);
      if (full.tin == full.tout || !live[size_t(full.joint)]) {
        CHECK(got.weight == 0.f && got.tin == got.tout && got.joint >= 0 && got.joint < Jc);
      } else {
        const int32_t c = cj(full.joint);
        CHECK(got.joint == c && got.parent == cr.parent[size_t(c)] && got.tin == ct.tin[size_t(c)] && got.tout == ct.tout[size_t(c)]);
      }
    }
  }
}

mmx::ProblemTopology positions(const Ints& pos, const Ints& ori = {}) {
  mmx::ProblemTopology p;
  p.Kp = int32_t(pos.size());
  p.Ko = int32_t(ori.size());
  p.posParent = pos;
  p.oriParent = ori;
  return p;
}

mmx_parameter_limit limit(int32_t type, int32_t index0, int32_t index1) {
  mmx_parameter_limit lm{};
  lm.type = type;
  lm.index0 = index0;
  lm.index1 = index1;
  lm.weight = 1.f;
  return lm;
}

mmx_ellipsoid_limit ellipsoid(int32_t parent, int32_t ellipsoidParent) {
  mmx_ellipsoid_limit e{};
  e.weight = 1.f;
  e.parent = parent;
  e.ellipsoid_parent = ellipsoidParent;
  return e;
}

} // namespace

int main() {
  const Ints chain7{-1, 0, 1, 2, 3, 4, 5}, star{-1, 0, 0, 0, 0, 0}, tree8{-1, 0, 1, 0, 3, 3, 0, 6}, twoRoots{-1, 0, 1, -1, 3, 4};
  checkCase("chain7, constraint mid-chain", treeRig(chain7), positions({3}));
  checkCase("chain7, everything live", treeRig(chain7), positions({6}, {2}));
  checkCase("star", treeRig(star), positions({4}, {2}));
  checkCase("tree8, dead subtree between live siblings", treeRig(tree8), positions({2, 7}));
  checkCase("two roots, first tree dead", treeRig(twoRoots), positions({5}));
  checkCase("two roots, second tree dead", treeRig(twoRoots), positions({1}, {1}));
  {
    mmx::ProblemTopology p = positions({4});
    p.instPos = true;
    p.unionPos = {1, 3};
    checkCase("star, per-instance position parents", treeRig(star), p);
    p = positions({3});
    p.hasModel = true;
    checkCase("chain7, model-parameter block", treeRig(chain7), p);
  }
  {
    // two branches of 10 and 9 joints below a root; parameter 20 is shared by joints 3 and 7 of the first branch: 21 solved
    // columns = two 16-blocks
    Ints parent{-1};
    for (int32_t j = 1; j < 20; ++j) {
      parent.push_back(j == 11 ? 0 : j - 1);
    }
    const Rig rig = treeRig(parent, {Triplet{7 * 3 + 4, 20, 0.5f}, Triplet{7 * 7 + 4, 20, -0.25f}}, 1);
    checkCase("branch20, one shared parameter", rig, positions({10, 19}, {15}));
    std::vector<uint8_t> enabled(21, 1);
    enabled[12] = 0, enabled[5] = 0;
    checkCase("branch20, enabled subset, short constraints", rig, positions({8, 14}), enabled);
  }
  {
    // 9-joint chain; parameter 9 has four sources, parameter 10 three: their H entry has 4 x 3 - 1 = 11 terms > 8
    const Ints chain9{-1, 0, 1, 2, 3, 4, 5, 6, 7};
    std::vector<Triplet> shared;
    for (int32_t j : {1, 3, 5, 7}) {
      shared.push_back(Triplet{7 * j + 4, 9, 0.5f});
    }
    for (int32_t j : {2, 4, 6}) { // (the middle one a translation: it moves points only)
      shared.push_back(Triplet{7 * j + (j == 4 ? 0 : 5), 10, 0.25f});
    }
    checkCase("chain9, two shared parameters, split entries", treeRig(chain9, shared, 2), positions({8}));
    checkCase("chain9, orientation below the translation source", treeRig(chain9, shared, 2), positions({2}, {6}));
  }
  {
    mmx::ProblemTopology p = positions({3});
    p.limits = {limit(MMX_LIMIT_MINMAX, 2, 0), limit(MMX_LIMIT_LINEAR, 1, 4), limit(MMX_LIMIT_LINEAR_JOINT, 7 * 2 + 3, 7 * 5 + 3)};
    checkCase("chain7, limits of three types", treeRig(chain7), p);
    p = positions({2, 7});
    p.limits = {limit(MMX_LIMIT_LINEAR, 2, 7), limit(MMX_LIMIT_LINEAR, 7, 2), limit(MMX_LIMIT_LINEAR_JOINT, 7 * 4 + 3, 7 * 1 + 3)};
    checkCase("tree8, limits across branches", treeRig(tree8), p);
  }
  {
    mmx::ProblemTopology p = positions({1});
    p.blocks.push_back({MMX_JC_FIXED_AXIS_COS, {4}, {}});
    p.blocks.push_back({MMX_JC_JOINT_TO_JOINT_DISTANCE, {2}, {7}});
    checkCase("tree8, fixed-axis block and pair block", treeRig(tree8), p);
  }
  {
    mmx::ProblemTopology p = positions({1});
    p.ellipsoids = {ellipsoid(5, 2)};
    checkCase("chain7, ellipsoid parent on the chain", treeRig(chain7), p);
    p.ellipsoids = {ellipsoid(7, 4)};
    checkCase("tree8, ellipsoid parent off the chain", treeRig(tree8), p);
  }
  std::printf("OK\n");
  return 0;
}
