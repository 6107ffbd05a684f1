// The rig-level tables of mmx_eval_skeleton_state_backward (buildStateBackwardTables, momentum_amd/csrc/mmx_host_tables.hpp)
// against restatements written here: the per-parameter source lists against a brute-force transpose of the CSR transform, entry
// for entry and in row order; the DFS order against a recursive pre-order walk; and the LDS budget rule (stateBackwardRefusal,
// mmx_solve_plan.hpp).  Stand-alone: links the two host files only, needs no GPU (tests/test_state_backward_tables_host.py builds
// it with the address and undefined-behaviour sanitizers).
#include "../../momentum_amd/csrc/mmx_host_tables.hpp"
#include "../../momentum_amd/csrc/mmx_solve_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace {

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
  int32_t joint, dof, param;
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

// CSR with ascending rows; within a row the entries keep the order they are given in
Rig makeRig(const Ints& parent, const std::vector<Triplet>& trip, int32_t P) {
  Rig r;
  r.J = int32_t(parent.size());
  r.P = P;
  r.parent = parent;
  r.ptOuter.assign(size_t(7 * r.J) + 1, 0);
  for (int32_t row = 0; row < 7 * r.J; ++row) {
    for (const Triplet& t : trip) {
      if (7 * t.joint + t.dof == row) {
        r.ptInner.push_back(t.param);
        r.ptValue.push_back(t.value);
      }
    }
    r.ptOuter[size_t(row) + 1] = int32_t(r.ptInner.size());
  }
  r.ptOffsets.assign(size_t(7 * r.J), 0.f);
  r.preRot.assign(size_t(4 * r.J), 0.f);
  r.offset.assign(size_t(3 * r.J), 0.f);
  for (int32_t j = 0; j < r.J; ++j) {
    r.preRot[size_t(4 * j + 3)] = 1.f;
  }
  return r;
}

void checkRig(const char* name, const Rig& rig) {
  g_case = name;
  const mmx_rig_desc d = rig.desc();
  mmx::HostTables all;
  std::string err;
  CHECK(mmx::buildHostTables(&d, nullptr, all, err) == MMX_OK);
  const mmx::StateBackwardTables t = mmx::buildStateBackwardTables(all);
  const int32_t J = rig.J, P = rig.P;
  // ---- DFS pre-order by a recursive walk, children in index order
  Ints order, pos(size_t(J), -1), size(size_t(J), 0);
  std::function<int32_t(int32_t)> walk = [&](int32_t j) {
    pos[size_t(j)] = int32_t(order.size());
    order.push_back(j);
    int32_t n = 1;
    for (int32_t c = j + 1; c < J; ++c) {
      if (rig.parent[size_t(c)] == j) {
        n += walk(c);
      }
    }
    size[size_t(j)] = n;
    return n;
  };
  for (int32_t j = 0; j < J; ++j) {
    if (rig.parent[size_t(j)] < 0) {
      walk(j);
    }
  }
  CHECK(int32_t(order.size()) == J);
  CHECK(t.dfsJoint == order);
  CHECK(t.jointPos == pos);
  CHECK(int32_t(t.subSize.size()) == J && int32_t(t.loadedPos.size()) == J);
  for (int32_t k = 0; k < J; ++k) {
    CHECK(t.subSize[size_t(k)] == size[size_t(order[size_t(k)])]);
    CHECK(t.loadedPos[size_t(k)] == k); // every position is a loaded one
  }
  // ---- the transpose of the transform, by brute force: per parameter, rows ascending, a row's entries in their order
  CHECK(int32_t(t.colStart.size()) == P + 1 && t.colStart[0] == 0);
  size_t total = 0;
  for (int32_t p = 0; p < P; ++p) {
    size_t e = size_t(t.colStart[size_t(p)]);
    for (int32_t row = 0; row < 7 * J; ++row) {
      for (int32_t k = rig.ptOuter[size_t(row)]; k < rig.ptOuter[size_t(row) + 1]; ++k) {
        if (rig.ptInner[size_t(k)] != p) {
          continue;
        }
        CHECK(e < t.colSources.size());
        const mmx::ColumnSource& s = t.colSources[e++];
        const int32_t joint = row / 7;
        CHECK(s.joint == joint && s.dof == row % 7 && s.parent == rig.parent[size_t(joint)]);
        CHECK(std::memcmp(&s.weight, &rig.ptValue[size_t(k)], sizeof(float)) == 0);
        CHECK(s.tin == pos[size_t(joint)] && s.tout == pos[size_t(joint)] + size[size_t(joint)]);
        ++total;
      }
    }
    CHECK(e == size_t(t.colStart[size_t(p) + 1]));
  }
  CHECK(total == rig.ptInner.size() && total == t.colSources.size());
}

} // namespace

int main() {
  // a parameter drives three dofs on different joints with weights != 1 (and the joints sit on different branches)
  checkRig("three dofs", makeRig({-1, 0, 1, 0, 3}, {{2, 5, 0, 0.7f}, {1, 3, 0, -1.3f}, {4, 6, 0, 0.4f}, {0, 0, 1, 1.f}, {3, 4, 2, 1.f}}, 3));
  // a dof is driven by two parameters (the entries of the row in descending parameter order, too)
  checkRig("two parameters", makeRig({-1, 0, 0, 2}, {{3, 5, 1, 0.6f}, {3, 5, 0, -0.8f}, {1, 4, 1, 2.f}, {0, 6, 2, 1.f}}, 3));
  // a parameter drives nothing (the first, one in the middle and the last)
  {
    const Rig rig = makeRig({-1, 0, 1}, {{0, 3, 1, 1.f}, {2, 4, 3, 0.5f}, {1, 0, 3, 0.25f}}, 5);
    checkRig("empty columns", rig);
    const mmx_rig_desc d = rig.desc();
    mmx::HostTables all;
    std::string err;
    CHECK(mmx::buildHostTables(&d, nullptr, all, err) == MMX_OK);
    const mmx::StateBackwardTables t = mmx::buildStateBackwardTables(all);
    CHECK(t.colStart == Ints({0, 0, 1, 1, 3, 3}));
  }
  // two roots, a zero stored value kept
  checkRig("two roots", makeRig({-1, -1, 1, 0}, {{2, 3, 0, 0.f}, {3, 1, 0, 1.5f}}, 2));
  // ---- the budget rule
  g_case = "budget";
  CHECK(mmx::stateBackwardRefusal(0) == nullptr);
  CHECK(mmx::stateBackwardRefusal(mmx::kPlanLdsBudget - 64) == nullptr);
  const char* why = mmx::stateBackwardRefusal(mmx::kPlanLdsBudget - 60);
  CHECK(why != nullptr && std::strstr(why, "LDS budget") != nullptr && std::strstr(why, "mmx_eval_skeleton_state_backward") != nullptr);
  CHECK(mmx::stateBackwardRefusal(size_t(1) << 20) != nullptr);
  std::printf("OK\n");
  return 0;
}
