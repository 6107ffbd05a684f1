// The tables of the skinning backward pass (buildSkinTables, momentum_amd/csrc/mmx_skin_tables.hpp) against restatements
// written here: the joint-sorted influence list against a std::stable_sort by joint of the (vertex, slot) pairs taken in
// order, entryWeight bit for bit against the weight it names, and the wave partition's properties -- it covers 0 .. J in
// strictly increasing steps, no wave costs more than the heaviest single joint, and no wave could have taken the next joint
// too (greedy-maximal).  Stand-alone: links mmx_skin_tables.cpp only, needs no GPU (tests/test_skin_tables_host.py builds it
// with the address and undefined-behaviour sanitizers).
#include "../../momentum_amd/csrc/mmx_skin_tables.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>

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

struct Skin {
  int32_t J = 0, V = 0, K = 0;
  Ints joint; // [V][K]
  std::vector<float> weight; // [V][K]
  mmx_skin_desc desc() const {
    mmx_skin_desc d{};
    d.num_vertices = V;
    d.max_influences = K;
    d.joint = joint.data();
    d.weight = weight.data();
    return d;
  }
};

// K = 1, weight 0.5: counts[j] vertices on joint j, vertex order shuffled
Skin listSkin(const Ints& counts, unsigned seed) {
  Skin s;
  s.J = int32_t(counts.size());
  s.K = 1;
  for (int32_t j = 0; j < s.J; ++j) {
    s.joint.insert(s.joint.end(), size_t(counts[size_t(j)]), j);
  }
  std::mt19937 rng(seed);
  std::shuffle(s.joint.begin(), s.joint.end(), rng);
  s.V = int32_t(s.joint.size());
  s.weight.assign(s.joint.size(), 0.5f);
  return s;
}

// zeroShare of the slots are padding: half of it +0, half of it -0; the other weights in +-[2^-149, 2)
Skin randomSkin(int32_t J, int32_t V, int32_t K, double zeroShare, unsigned seed) {
  Skin s;
  s.J = J, s.V = V, s.K = K;
  std::mt19937 rng(seed);
  std::uniform_int_distribution<int32_t> anyJoint(0, J - 1);
  std::uniform_real_distribution<double> unit(0.0, 1.0);
  for (int32_t i = 0; i < V * K; ++i) {
    s.joint.push_back(anyJoint(rng));
    float w = unit(rng) < 0.05 ? 1e-45f : float(0.01 + 1.99 * unit(rng));
    w = unit(rng) < 0.3 ? -w : w;
    if (unit(rng) < zeroShare) {
      w = unit(rng) < 0.5 ? 0.f : -0.f;
    }
    s.weight.push_back(w);
  }
  return s;
}

mmx::SkinTables checkSkin(const char* name, const Skin& s) {
  g_case = name;
  const mmx_skin_desc d = s.desc();
  std::string err;
  CHECK(mmx::validateSkinDesc(s.J, &d, false, err) == MMX_OK);
  const mmx::SkinTables t = mmx::buildSkinTables(s.J, &d);
  const int32_t J = s.J;
  // ---- the influence list: the non-zero-weight (v, k) pairs in order, stable-sorted by joint
  Ints pairs;
  for (int32_t i = 0; i < s.V * s.K; ++i) {
    if (s.weight[size_t(i)] != 0.f) {
      pairs.push_back(i);
    }
  }
  std::stable_sort(pairs.begin(), pairs.end(), [&](int32_t a, int32_t b) { return s.joint[size_t(a)] < s.joint[size_t(b)]; });
  const size_t E = pairs.size();
  CHECK(t.entryVertex.size() == E && t.entrySlot.size() == E && t.entryWeight.size() == E);
  CHECK(int32_t(t.jointStart.size()) == J + 1 && t.jointStart[0] == 0 && size_t(t.jointStart[size_t(J)]) == E);
  Ints count(size_t(J), 0);
  for (size_t e = 0; e < E; ++e) {
    const int32_t v = pairs[e] / s.K, k = pairs[e] % s.K;
    CHECK(t.entryVertex[e] == v && t.entrySlot[e] == k);
    const float w = s.weight[size_t(t.entryVertex[e]) * size_t(s.K) + size_t(t.entrySlot[e])];
    CHECK(std::memcmp(&t.entryWeight[e], &w, sizeof(float)) == 0);
    CHECK(t.entryWeight[e] != 0.f);
    const int32_t j = s.joint[size_t(pairs[e])];
    CHECK(int32_t(e) >= t.jointStart[size_t(j)] && int32_t(e) < t.jointStart[size_t(j) + 1]);
    ++count[size_t(j)];
  }
  for (int32_t j = 0; j < J; ++j) {
    CHECK(t.jointStart[size_t(j) + 1] - t.jointStart[size_t(j)] == count[size_t(j)]);
  }
  // ---- the wave partition
  auto cost = [&](int32_t j0, int32_t j1) { // of the joints j0 .. j1 - 1
    int64_t c = 0;
    for (int32_t j = j0; j < j1; ++j) {
      c += int64_t(count[size_t(j)]) + mmx::kSkinJointCost;
    }
    return c;
  };
  int64_t heaviest = 0;
  for (int32_t j = 0; j < J; ++j) {
    heaviest = std::max(heaviest, cost(j, j + 1));
  }
  const Ints& ws = t.waveStart;
  CHECK(ws.size() >= 2 && ws.front() == 0 && ws.back() == J);
  for (size_t w = 0; w + 1 < ws.size(); ++w) {
    CHECK(ws[w] < ws[w + 1]); // strictly increasing: every joint in exactly one wave, no empty wave
    CHECK(cost(ws[w], ws[w + 1]) <= heaviest);
    if (w + 2 < ws.size()) {
      CHECK(cost(ws[w], ws[w + 1] + 1) > heaviest); // greedy-maximal: the next wave's first joint did not fit
    }
  }
  return t;
}

} // namespace

int main() {
  // ---- seeded random skins: J 1 .. 40, K 1 .. 8, zero-weight shares from 0 to 1
  const double shares[] = {0.0, 0.1, 0.25, 0.5, 0.9, 0.99, 1.0};
  unsigned seed = 1;
  for (int32_t J = 1; J <= 40; ++J) {
    for (int32_t K = 1; K <= 8; ++K) {
      const double share = shares[(J + K) % 7];
      const int32_t V = 1 + int32_t((seed * 37u) % 200u);
      char name[64];
      std::snprintf(name, sizeof name, "random J=%d K=%d V=%d zero=%.2f", J, K, V, share);
      checkSkin(name, randomSkin(J, V, K, share, seed++));
    }
  }
  // skewed: most entries on one joint, so that many light joints are packed behind it
  for (int32_t heavy : {0, 7, 19}) {
    Skin s = randomSkin(20, 600, 3, 0.2, 1000u + unsigned(heavy));
    for (size_t i = 0; i < s.joint.size(); i += 2) {
      s.joint[i] = heavy;
    }
    checkSkin("skewed", s);
  }
  // ---- every weight zero (of either sign): no entries, one wave over all joints
  {
    const mmx::SkinTables t = checkSkin("all zero", randomSkin(9, 50, 4, 1.0, 77));
    CHECK(t.entryVertex.empty() && t.waveStart == Ints({0, 1, 2, 3, 4, 5, 6, 7, 8, 9}));
    // (every joint costs kSkinJointCost, the heaviest single joint's: one joint per wave)
  }
  // ---- the first and the last joint empty
  {
    const mmx::SkinTables t = checkSkin("ends empty", listSkin({0, 30, 2, 5, 0}, 3));
    CHECK(t.jointStart == Ints({0, 0, 30, 32, 37, 37}));
    CHECK(t.waveStart == Ints({0, 1, 2, 4, 5})); // costs 16 | 46 | 18 + 21 | 16, heaviest 46
  }
  // ---- an exact fit is taken: costs 32 | 16 + 16, heaviest 32
  {
    const mmx::SkinTables t = checkSkin("exact fit", listSkin({16, 0, 0}, 8));
    CHECK(t.waveStart == Ints({0, 1, 3}));
  }
  // ---- one joint, one entry
  {
    const mmx::SkinTables t = checkSkin("one entry", listSkin({1}, 4));
    CHECK(t.waveStart == Ints({0, 1}));
  }
  // ---- the list-length skin of tests/test_gpu_skin_points_entries.py: lists at 1, 63/64/65, 255/256/257, 511/512/513 and
  // empty joints packed into waves 0 and 3
  {
    const mmx::SkinTables t = checkSkin("list lengths", listSkin({0, 1, 63, 64, 65, 0, 255, 256, 257, 0, 0, 511, 512, 513, 0, 0}, 5));
    CHECK(t.entryVertex.size() == 2497);
    CHECK(t.waveStart == Ints({0, 6, 7, 8, 11, 12, 13, 14, 16}));
  }
  // ---- equal lists of 40: a wave per joint, so J waves -- every residue modulo the four waves of a workgroup
  for (int32_t J : {1, 2, 3, 5, 6, 7}) {
    const mmx::SkinTables t = checkSkin("equal lists", listSkin(Ints(size_t(J), 40), 6u + unsigned(J)));
    Ints each(size_t(J) + 1);
    std::iota(each.begin(), each.end(), 0);
    CHECK(t.waveStart == each);
  }
  std::printf("OK\n");
  return 0;
}
