// mmx_skin_tables.cpp -- the joint-sorted influence list and the wave partition of linear-blend skinning (mmx_skin_tables.hpp).
#include "mmx_skin_tables.hpp"

#include <algorithm>
#include <cmath>

namespace mmx {

const char* skinRefusal(int32_t J) {
  if (skinLdsBytes(J) > size_t(160) * 1024 - 64) {
    return "mmx_skin_create: the rig's posed affines (48 bytes per joint) do not fit the kernels' LDS budget (160 KB)";
  }
  return nullptr;
}

int32_t validateSkinDesc(int32_t J, const mmx_skin_desc* d, bool payload, std::string& err) {
  auto bad = [&](const char* what) {
    err = std::string("skin descriptor: ") + what;
    return int32_t(MMX_ERR_INVALID_ARGUMENT);
  };
  if (d == nullptr) {
    return bad("descriptor is null");
  }
  if (J < 1) {
    return bad("num_joints must be >= 1");
  }
  if (d->num_vertices < 1) {
    return bad("num_vertices must be >= 1");
  }
  if (d->max_influences < 1 || d->max_influences > MMX_MAX_SKIN_INFLUENCES) {
    return bad("max_influences must be in 1 .. MMX_MAX_SKIN_INFLUENCES (8)");
  }
  if (d->joint == nullptr || d->weight == nullptr) {
    return bad("joint / weight is null");
  }
  if (size_t(d->num_vertices) * size_t(d->max_influences) > size_t(INT32_MAX)) {
    return bad("num_vertices * max_influences exceeds 2^31 - 1");
  }
  const size_t n = size_t(d->num_vertices) * size_t(d->max_influences);
  for (size_t i = 0; i < n; ++i) {
    if (d->joint[i] < 0 || d->joint[i] >= J) {
      return bad("joint index out of range (zero-weight slots carry a valid index too)");
    }
    if (!std::isfinite(d->weight[i])) {
      return bad("non-finite weight");
    }
  }
  if (payload) {
    if (d->rest_positions == nullptr) {
      return bad("rest_positions is null");
    }
    for (size_t i = 0; i < size_t(d->num_vertices) * 3; ++i) {
      if (!std::isfinite(d->rest_positions[i])) {
        return bad("non-finite rest position");
      }
    }
    for (size_t i = 0; d->inverse_bind != nullptr && i < size_t(J) * 12; ++i) {
      if (!std::isfinite(d->inverse_bind[i])) {
        return bad("non-finite inverse-bind entry");
      }
    }
  }
  return MMX_OK;
}

SkinTables buildSkinTables(int32_t J, const mmx_skin_desc* d) {
  SkinTables t;
  const int32_t V = d->num_vertices, K = d->max_influences;
  // counting sort by joint; vertices and slots are visited in ascending order, so each joint's entries come out sorted
  t.jointStart.assign(size_t(J) + 1, 0);
  for (size_t i = 0; i < size_t(V) * size_t(K); ++i) {
    if (d->weight[i] != 0.f) {
      ++t.jointStart[size_t(d->joint[i]) + 1];
    }
  }
  for (int32_t j = 0; j < J; ++j) {
    t.jointStart[size_t(j) + 1] += t.jointStart[size_t(j)];
  }
  const size_t E = size_t(t.jointStart[size_t(J)]);
  t.entryVertex.resize(E), t.entrySlot.resize(E), t.entryWeight.resize(E);
  std::vector<int32_t> next(t.jointStart.begin(), t.jointStart.end() - 1);
  for (int32_t v = 0; v < V; ++v) {
    for (int32_t k = 0; k < K; ++k) {
      const size_t i = size_t(v) * size_t(K) + size_t(k);
      if (d->weight[i] != 0.f) {
        const size_t e = size_t(next[size_t(d->joint[i])]++);
        t.entryVertex[e] = v, t.entrySlot[e] = k, t.entryWeight[e] = d->weight[i];
      }
    }
  }
  // the wave partition
  auto cost = [&](int32_t j) { return int64_t(t.jointStart[size_t(j) + 1] - t.jointStart[size_t(j)]) + kSkinJointCost; };
  int64_t heaviest = 0;
  for (int32_t j = 0; j < J; ++j) {
    heaviest = std::max(heaviest, cost(j));
  }
  t.waveStart.push_back(0);
  int64_t load = 0;
  for (int32_t j = 0; j < J; ++j) {
    if (load > 0 && load + cost(j) > heaviest) {
      t.waveStart.push_back(j);
      load = 0;
    }
    load += cost(j);
  }
  t.waveStart.push_back(J);
  return t;
}

} // namespace mmx
