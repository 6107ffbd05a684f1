// adapter_projection.cpp -- a projection + distance batch through integration/tensor_ik_mmx_adapter.cpp's solveBatch on
// momentum's three-joint test character (the shape of integration/adapter_check.cpp).  Writes the inputs it made up and the
// solved parameters to the file named by argv[1] (float32, in the order tests/test_adapter_projection.py reads them), so
// that the test can send the same problem through momentum_amd.capi and compare bit for bit.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tensor_ik_mmx_adapter.h"

static momentum::Character testCharacter() {
  momentum::Character c;
  const char* names[3] = {"root", "joint1", "joint2"};
  for (int j = 0; j < 3; ++j) {
    momentum::Joint jt;
    jt.name = names[j];
    jt.parent = j == 0 ? momentum::kInvalidIndex : size_t(j - 1);
    jt.translationOffset.v[1] = j == 0 ? 0.f : 1.f;
    c.skeleton.joints.push_back(jt);
  }
  auto& pt = c.parameterTransform;
  pt.name = {"root_tx", "root_ty", "root_tz", "root_rx", "root_ry", "root_rz", "scale_global", "joint1_rx", "shared_rz", "joint2_rx"};
  const int rowOf[11] = {0, 1, 2, 3, 4, 5, 6, 7 + 3, 7 + 5, 14 + 3, 14 + 5};
  const int colOf[11] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8};
  const float valOf[11] = {1, 1, 1, 1, 1, 1, 1, 1, 0.5f, 1, 0.5f};
  pt.transform.outer.assign(1, 0);
  for (int r = 0; r < 21; ++r) {
    for (int k = 0; k < 11; ++k) {
      if (rowOf[k] == r) {
        pt.transform.inner.push_back(colOf[k]);
        pt.transform.values.push_back(valOf[k]);
      }
    }
    pt.transform.outer.push_back(int(pt.transform.inner.size()));
  }
  pt.offsets.v.assign(21, 0.f);
  return c;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: adapter_projection OUT\n");
    return 2;
  }
  if (mmx_device_count() <= 0) {
    std::printf("no device\n");
    return 3;
  }
  const int B = 8, Kp = 1, Kq = 3, Kd = 1, P = 10;
  const int32_t posParents[Kp] = {2}, projParents[Kq] = {1, 2, 2}, distParents[Kd] = {2};
  std::vector<float> posOff(B * Kp * 3, 0.f), posTgt(B * Kp * 3), posW(B * Kp, 1.f);
  std::vector<float> projOff(B * Kq * 3, 0.f), proj(B * Kq * 12), projTgt(B * Kq * 2), projW(B * Kq, 1.f);
  std::vector<float> distOff(B * Kd * 3, 0.f), distOrigin(B * Kd * 3), distTgt(B * Kd), distW(B * Kd, 1.f), theta(B * P, 0.f);
  for (int b = 0; b < B; ++b) {
    posTgt[3 * b] = 0.1f * float(b), posTgt[3 * b + 1] = 2.2f, posTgt[3 * b + 2] = -0.05f * float(b);
    for (int k = 0; k < Kq; ++k) {
      // a camera at (0, 1, -4 - 0.1 b) looking along +z with focal length 3 (a third of them turned away: clipped)
      float* m = &proj[size_t(12 * (Kq * b + k))];
      const float away = (k == 2 && b % 3 == 0) ? -1.f : 1.f, f = 3.f, ez = -4.f - 0.1f * float(b);
      const float row[12] = {away * f, 0.f, 0.f, 0.f, 0.f, f, 0.f, -f, 0.f, 0.f, away, -away * ez};
      for (int q = 0; q < 12; ++q) {
        m[q] = row[q];
      }
      projOff[size_t(3 * (Kq * b + k) + 1)] = 0.25f * float(k);
      projTgt[size_t(2 * (Kq * b + k))] = 0.05f * float(k + b % 4);
      projTgt[size_t(2 * (Kq * b + k) + 1)] = 0.3f - 0.02f * float(b);
    }
    distOrigin[3 * b] = 1.f, distOrigin[3 * b + 1] = 0.5f * float(b % 2), distOrigin[3 * b + 2] = 0.f;
    distTgt[b] = 1.5f + 0.05f * float(b);
  }
  mmx_adapter::BatchTensors t;
  t.nBatch = B, t.numPositions = Kp, t.positionParents = posParents;
  t.positionOffsets = posOff.data(), t.positionTargets = posTgt.data(), t.positionWeights = posW.data();
  t.numProjections = Kq, t.projectionParents = projParents, t.projectionOffsets = projOff.data(), t.projections = proj.data();
  t.projectionTargets = projTgt.data(), t.projectionWeights = projW.data(), t.projectionNearClip = 0.5f;
  t.numDistances = Kd, t.distanceParents = distParents, t.distanceOffsets = distOff.data(), t.distanceOrigins = distOrigin.data();
  t.distanceTargets = distTgt.data(), t.distanceWeights = distW.data();
  pymomentum::SolverOptions o;
  o.linearSolverType = pymomentum::LinearSolverType::QR, o.levmar_lambda = 0.05f, o.minIter = 6, o.maxIter = 6, o.threshold = 1.f, o.lineSearch = false;
  momentum::ParameterSet all;
  all.set();
  const momentum::Character c = testCharacter();
  mmx_rig* rig = mmx_adapter::makeRig(c, 0);
  const mmx_adapter::SolveReport rep = mmx_adapter::solveBatch(rig, all, t, o, theta.data(), MMX_PRECISION_F32);
  mmx_rig_destroy(rig);
  if (rep.failed != 0) {
    std::printf("FAIL: %lld elements failed\n", (long long)rep.failed);
    return 1;
  }
  FILE* f = std::fopen(argv[1], "wb");
  if (f == nullptr) {
    return 1;
  }
  for (const std::vector<float>* v : {&posTgt, &projOff, &proj, &projTgt, &distOrigin, &distTgt, &theta}) {
    std::fwrite(v->data(), sizeof(float), v->size(), f);
  }
  std::fclose(f);
  std::printf("OK\n");
  return 0;
}
