// mmx_eval_gradient's scope decision (gradientRefusal, momentum_amd/csrc/mmx_solve_plan.cpp) on the CPU: every refusal
// condition alone and in every pair -- the first in the documented order (include/mmx.h) is the one reported --, the all-clear
// case, and the edges of the LDS budget.  A stand-alone program that links the one host file and nothing else; built with the
// address and undefined-behaviour sanitizers by tests/test_gradient_plan_host.py.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../momentum_amd/csrc/mmx_solve_plan.hpp"

using mmx::SolveFacts;

static int bad = 0;

static void expect(const char* what, const char* got, const char* key) {
  const bool ok = key == nullptr ? got == nullptr : (got != nullptr && std::strstr(got, key) != nullptr && std::strstr(got, "mmx_eval_gradient") == got);
  if (!ok) {
    std::printf("FAIL %s: got \"%s\", expected %s%s\n", what, got != nullptr ? got : "(accepted)", key != nullptr ? "a refusal naming " : "acceptance", key != nullptr ? key : "");
    ++bad;
  }
}

static SolveFacts clear() {
  SolveFacts f;
  f.J = 72, f.U = 64, f.n = 110, f.M = 192 + 5 + 128, f.rowsJoint = 192;
  f.NL = 5, f.hasModel = 1; // the parameter-space rows are inside the scope
  f.lossPosType = 1, f.lossOriType = 3; // ... and so is every loss
  f.gradientLdsBytes = 24 * 1024;
  return f;
}

namespace {
struct Condition {
  const char* key; // what the message must name
  std::function<void(SolveFacts&)> trip;
};
} // namespace

int main() {
  // the documented order
  const std::vector<Condition> order = {
      {"joint-constraint blocks", [](SolveFacts& f) { f.numBlocks = 1, f.G = 3, f.GT = 3; }},
      {"ellipsoid limits", [](SolveFacts& f) { f.NE = 2, f.GT += 2; }},
      {"per-instance constraint parents", [](SolveFacts& f) { f.instanceParents = true; }},
      {"no position / orientation constraint, or no solved parameter", [](SolveFacts& f) { f.U = 0; }},
      {"LDS budget", [](SolveFacts& f) { f.gradientLdsBytes = mmx::kPlanLdsBudget; }},
  };
  expect("all clear", mmx::gradientRefusal(clear()), nullptr);
  for (size_t i = 0; i < order.size(); ++i) {
    SolveFacts f = clear();
    order[i].trip(f);
    expect(order[i].key, mmx::gradientRefusal(f), order[i].key);
    for (size_t j = 0; j < order.size(); ++j) {
      if (j == i) {
        continue;
      }
      SolveFacts g = clear();
      order[i].trip(g);
      order[j].trip(g);
      expect("pair", mmx::gradientRefusal(g), order[i < j ? i : j].key);
    }
  }
  { // the other spellings of a condition
    SolveFacts f = clear();
    f.G = 1; // constraints of a block without the block count
    expect("G alone", mmx::gradientRefusal(f), "joint-constraint blocks");
    f = clear();
    f.n = 0;
    expect("n = 0", mmx::gradientRefusal(f), "no solved parameter");
    f = clear();
    f.U = 0, f.n = 0;
    expect("U = n = 0", mmx::gradientRefusal(f), "no position / orientation constraint");
  }
  { // the budget's edge: 64 bytes stay with the runtime, as in the tree kernels' launchers
    SolveFacts f = clear();
    f.gradientLdsBytes = mmx::kPlanLdsBudget - 64;
    expect("budget - 64", mmx::gradientRefusal(f), nullptr);
    f.gradientLdsBytes = mmx::kPlanLdsBudget - 60;
    expect("budget - 60", mmx::gradientRefusal(f), "LDS budget");
    f.gradientLdsBytes = 0;
    expect("no LDS at all", mmx::gradientRefusal(f), nullptr);
  }
  { // what the solves refuse or route on does not matter here
    SolveFacts f = clear();
    f.route = MMX_ROUTE_WAVE, f.fusedUsable = false, f.treeUsable = false, f.fusedBlocks = -1, f.solveN = 4000, f.parameterHistory = true, f.stepHistory = true;
    expect("solve-only facts", mmx::gradientRefusal(f), nullptr);
  }
  // the new fact sits at the end of SolveFacts with a default that refuses nothing
  if (SolveFacts{}.gradientLdsBytes != 0) {
    std::printf("FAIL: SolveFacts::gradientLdsBytes default\n");
    ++bad;
  }
  if (bad != 0) {
    std::printf("FAIL: %d check(s)\n", bad);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
