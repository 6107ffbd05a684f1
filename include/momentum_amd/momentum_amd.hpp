// momentum_amd.hpp -- header-only C++17 shell over the C ABI (include/mmx.h) that keeps momentum's
// Character / Skeleton / SkeletonSolverFunction / GaussNewtonSolver surface for the batched IK
// path, so that code written against momentum's classes switches to the MI355X path by changing
// the namespace and the solver type.  Host-side glue only; all compute is in libmmx_hip.so.
//
// Mirrors (reference file:line):
//   Joint / Skeleton                 momentum/character/joint.h:18-36, skeleton.h:22-25
//   ParameterTransform               momentum/character/parameter_transform.h:62-95 (CSR = SparseRowMatrix)
//   Character                        momentum/character/character.h:32-125 (skeleton + parameterTransform only)
//   PositionData / OrientationData   momentum/character_solver/position_error_function.h:16-29,
//                                    orientation_error_function.h:16-36
//   SolverOptions                    momentum/solver/solver.h:19-34
//   GaussNewtonSolverOptions         momentum/solver/gauss_newton_solver.h:17-59
//   SkeletonSolverFunction           momentum/character_solver/skeleton_solver_function.h:21-95
//   GaussNewtonSolver::solve         momentum/solver/solver.cpp:50-128 (one per batch element, as
//                                    pymomentum/tensor_ik/tensor_ik.cpp:127-177 does)
// Errors: every non-zero status becomes std::runtime_error with the library's message, the
// OSS behaviour of MT_CHECK / MT_THROW (momentum/common/checks.h:36-45, exception.h:24-66).
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../mmx.h"

namespace momentum_amd {

inline constexpr size_t kInvalidIndex = std::numeric_limits<size_t>::max(); // character/types.h:182
inline constexpr size_t kParametersPerJoint = 7; // character/types.h:21

using Vector3f = std::array<float, 3>;
using Quaternionf = std::array<float, 4>; // (x, y, z, w), Eigen storage order
using ParameterSet = std::vector<bool>; // momentum: std::bitset<kMaxModelParams>

inline void check(int32_t rc) {
  if (rc != MMX_OK) {
    throw std::runtime_error(std::string("momentum_amd: ") + mmx_last_error());
  }
}

struct Joint {
  std::string name;
  size_t parent = kInvalidIndex;
  Quaternionf preRotation{0.f, 0.f, 0.f, 1.f};
  Vector3f translationOffset{0.f, 0.f, 0.f};
};

struct Skeleton {
  std::vector<Joint> joints;
};

// Row-major sparse 7J x P transform + offsets.  `addEntry` keeps rows sorted by column.
struct ParameterTransform {
  std::vector<std::string> name; // model parameter names; size = numAllModelParameters()
  std::vector<int32_t> outer{0}, inner;
  std::vector<float> value;
  std::vector<float> offsets;

  size_t numAllModelParameters() const {
    return name.size();
  }
  // build from (row, col, value) triplets like Eigen's setFromTriplets
  struct Triplet {
    int32_t row, col;
    float value;
  };
  void setFromTriplets(size_t numJoints, const std::vector<Triplet>& triplets) {
    const size_t rows = kParametersPerJoint * numJoints;
    std::vector<std::vector<std::pair<int32_t, float>>> r(rows);
    for (const auto& t : triplets) {
      if (t.row < 0 || size_t(t.row) >= rows || t.col < 0 || size_t(t.col) >= name.size()) {
        throw std::runtime_error("ParameterTransform triplet out of range");
      }
      bool merged = false;
      for (auto& e : r[t.row]) {
        if (e.first == t.col) {
          e.second += t.value;
          merged = true;
        }
      }
      if (!merged) {
        r[t.row].push_back({t.col, t.value});
      }
    }
    outer.assign(1, 0);
    inner.clear();
    value.clear();
    for (auto& row : r) {
      for (size_t i = 1; i < row.size(); ++i) { // insertion sort by column
        for (size_t j = i; j > 0 && row[j].first < row[j - 1].first; --j) {
          std::swap(row[j], row[j - 1]);
        }
      }
      for (const auto& e : row) {
        inner.push_back(e.first);
        value.push_back(e.second);
      }
      outer.push_back(int32_t(inner.size()));
    }
    offsets.assign(rows, 0.f);
  }
};

struct Character {
  Skeleton skeleton;
  ParameterTransform parameterTransform;
};

struct PositionData {
  Vector3f offset{0.f, 0.f, 0.f};
  Vector3f target{0.f, 0.f, 0.f};
  size_t parent = 0;
  float weight = 1.f;
};

// momentum::ParameterLimit restricted to the limit types that act on model parameters
// (momentum/character/parameter_limits.h:20-31,33-99,125-136)
enum LimitType {
  MinMax = MMX_LIMIT_MINMAX,
  MinMaxJoint = MMX_LIMIT_MINMAX_JOINT, // index0 = 7 * jointIndex + jointParameter
  Linear = MMX_LIMIT_LINEAR,
  LinearJoint = MMX_LIMIT_LINEAR_JOINT,
  HalfPlane = MMX_LIMIT_HALFPLANE
};
struct ParameterLimit {
  LimitType type = MinMax;
  float weight = 1.f;
  // MinMax: parameterIndex, limits = {min, max}
  // Linear: referenceIndex, targetIndex, {scale, offset, rangeMin, rangeMax}
  // HalfPlane: param1, param2, {normal[0], normal[1], offset}
  size_t index0 = 0, index1 = 0;
  std::array<float, 4> values{0.f, 0.f, 0.f, 0.f};
  static ParameterLimit minMax(size_t parameterIndex, float lo, float hi, float weight = 1.f) {
    return ParameterLimit{MinMax, weight, parameterIndex, 0, {lo, hi, 0.f, 0.f}};
  }
  static ParameterLimit
  linear(size_t referenceIndex, size_t targetIndex, float scale, float offset, float rangeMin = 0.f, float rangeMax = 0.f, float weight = 1.f) {
    return ParameterLimit{Linear, weight, referenceIndex, targetIndex, {scale, offset, rangeMin, rangeMax}};
  }
  static ParameterLimit halfPlane(size_t param1, size_t param2, float n0, float n1, float offset, float weight = 1.f) {
    return ParameterLimit{HalfPlane, weight, param1, param2, {n0, n1, offset, 0.f}};
  }
};
using ParameterLimits = std::vector<ParameterLimit>;

struct OrientationData {
  Quaternionf offset{0.f, 0.f, 0.f, 1.f};
  Quaternionf target{0.f, 0.f, 0.f, 1.f};
  size_t parent = 0;
  float weight = 1.f;
};

struct SolverOptions {
  size_t minIterations = 1;
  size_t maxIterations = 2;
  float threshold = 1.0f;
  bool verbose = false;
  virtual ~SolverOptions() = default;
};

// gauss_newton_solver.h:17-33
struct GaussNewtonSolverBaseOptions : SolverOptions {
  float regularization = 0.05f;
  bool doLineSearch = false;
  GaussNewtonSolverBaseOptions() = default;
  /* implicit */ GaussNewtonSolverBaseOptions(const SolverOptions& base) : SolverOptions(base) {}
};

struct GaussNewtonSolverOptions : GaussNewtonSolverBaseOptions {
  bool useBlockJtJ = false; // accepted for source compatibility: both settings build the same system
  GaussNewtonSolverOptions() = default;
  explicit GaussNewtonSolverOptions(const SolverOptions& base) : GaussNewtonSolverBaseOptions(base) {}
};

// subset_gauss_newton_solver.h:19-26 and gauss_newton_solver_qr.h:20-25: the two solvers the batched
// driver builds (pymomentum/tensor_ik/tensor_ik.cpp:142-158).  Same normal equations as
// GaussNewtonSolverT; their line search tests against the directional derivative
// (MMX_LINE_SEARCH_DIRECTIONAL).
struct SubsetGaussNewtonSolverOptions : GaussNewtonSolverBaseOptions {
  SubsetGaussNewtonSolverOptions() = default;
  /* implicit */ SubsetGaussNewtonSolverOptions(const SolverOptions& base) : GaussNewtonSolverBaseOptions(base) {}
};
struct GaussNewtonSolverQROptions : GaussNewtonSolverBaseOptions {
  GaussNewtonSolverQROptions() = default;
  /* implicit */ GaussNewtonSolverQROptions(const SolverOptions& base) : GaussNewtonSolverBaseOptions(base) {}
};
// trust_region_qr.h:22-33: the third solver the batched driver builds (tensor_ik.cpp:150-152)
struct TrustRegionQROptions : SolverOptions {
  float trustRegionRadius_ = 1.0f;
  TrustRegionQROptions() = default;
  /* implicit */ TrustRegionQROptions(const SolverOptions& base) : SolverOptions(base) {}
};

// Device-resident Skeleton + ParameterTransform.
class DeviceCharacter {
 public:
  explicit DeviceCharacter(const Character& c, int device = 0) : numJoints_(c.skeleton.joints.size()) {
    const size_t J = numJoints_;
    std::vector<int32_t> parent(J);
    std::vector<float> pre(4 * J), off(3 * J);
    for (size_t j = 0; j < J; ++j) {
      const Joint& jt = c.skeleton.joints[j];
      parent[j] = jt.parent == kInvalidIndex ? MMX_INVALID_PARENT : int32_t(jt.parent);
      for (int k = 0; k < 4; ++k) {
        pre[4 * j + k] = jt.preRotation[k];
      }
      for (int k = 0; k < 3; ++k) {
        off[3 * j + k] = jt.translationOffset[k];
      }
    }
    const ParameterTransform& pt = c.parameterTransform;
    if (pt.outer.size() != kParametersPerJoint * J + 1) {
      throw std::runtime_error("momentum_amd: parameter transform has the wrong number of rows");
    }
    mmx_rig_desc d{};
    d.num_joints = int32_t(J);
    d.num_params = int32_t(pt.numAllModelParameters());
    d.parent = parent.data();
    d.pre_rotation = pre.data();
    d.translation_offset = off.data();
    d.pt_outer = pt.outer.data();
    d.pt_inner = pt.inner.data();
    d.pt_value = pt.value.data();
    d.pt_offsets = pt.offsets.empty() ? nullptr : pt.offsets.data();
    numParams_ = pt.numAllModelParameters();
    parents_ = parent;
    mmx_rig* h = nullptr;
    check(mmx_rig_create(&d, device, &h));
    handle_.reset(h, [](mmx_rig* p) { mmx_rig_destroy(p); });
  }
  mmx_rig* handle() const {
    return handle_.get();
  }
  size_t numParameters() const {
    return numParams_;
  }
  size_t numJoints() const {
    return numJoints_;
  }
  int32_t parentOf(size_t joint) const { // MMX_INVALID_PARENT for a root
    return parents_[joint];
  }

 private:
  std::shared_ptr<mmx_rig> handle_;
  size_t numJoints_ = 0, numParams_ = 0;
  std::vector<int32_t> parents_;
};

// Constraint data of the further JointErrorFunction specialisations; vectors are normalised where
// the reference's constructors do (plane_error_function.h:16-31, aim_error_function.h:17-37,
// fixed_axis_error_function.h:17-31, normal_error_function.h:17-36).
struct PlaneData {
  Vector3f offset{0.f, 0.f, 0.f};
  Vector3f normal{0.f, 1.f, 0.f};
  float d = 0.f;
  size_t parent = 0;
  float weight = 1.f;
};
struct AimData {
  Vector3f localPoint{0.f, 0.f, 0.f};
  Vector3f localDir{0.f, 0.f, 1.f};
  Vector3f globalTarget{0.f, 0.f, 0.f};
  size_t parent = 0;
  float weight = 1.f;
};
struct FixedAxisData {
  Vector3f localAxis{0.f, 0.f, 1.f};
  Vector3f globalAxis{0.f, 0.f, 1.f};
  size_t parent = 0;
  float weight = 1.f;
};
struct NormalData {
  Vector3f localPoint{0.f, 0.f, 0.f};
  Vector3f localNormal{0.f, 0.f, 1.f};
  Vector3f globalPoint{0.f, 0.f, 0.f};
  size_t parent = 0;
  float weight = 1.f;
};
// ABI 12's two point functions and the pair function (include/mmx.h: restated without file:line citations)
struct ProjectionData {
  std::array<float, 12> projection{{1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f}}; // 3 x 4 row-major camera matrix
  Vector3f offset{0.f, 0.f, 0.f};
  std::array<float, 2> target{{0.f, 0.f}}; // (u, v)
  size_t parent = 0;
  float weight = 1.f;
};
struct DistanceData {
  Vector3f origin{0.f, 0.f, 0.f};
  float target = 0.f; // target distance
  Vector3f offset{0.f, 0.f, 0.f};
  size_t parent = 0;
  float weight = 1.f;
};
struct JointToJointDistanceData {
  size_t joint1 = 0;
  Vector3f offset1{0.f, 0.f, 0.f};
  size_t joint2 = 0;
  Vector3f offset2{0.f, 0.f, 0.f};
  float targetDistance = 0.f;
  float weight = 1.f;
};
enum class JointErrorFunctionType {
  Plane = MMX_JC_PLANE, // PlaneErrorFunction(above = false)
  HalfPlane = MMX_JC_HALF_PLANE, // PlaneErrorFunction(above = true)
  AimDist = MMX_JC_AIM_DIST,
  AimDir = MMX_JC_AIM_DIR,
  FixedAxisDiff = MMX_JC_FIXED_AXIS_DIFF,
  FixedAxisCos = MMX_JC_FIXED_AXIS_COS,
  FixedAxisAngle = MMX_JC_FIXED_AXIS_ANGLE,
  Normal = MMX_JC_NORMAL,
  Projection = MMX_JC_PROJECTION, // L2 loss only, like the next two
  Distance = MMX_JC_DISTANCE,
  JointToJointDistance = MMX_JC_JOINT_TO_JOINT_DISTANCE // added with addJointToJointDistanceErrorFunction (two parent lists)
};

// One SkeletonSolverFunction + PositionErrorFunction + OrientationErrorFunction per batch element.
// The parent lists of the constructor are the default of every element; an element whose constraints name
// other parents (ConstraintData::parent) gets its own list, and setCharacters() gives every element its own
// Character of the same topology -- what solveTensorIKProblem does with characters[iBatch]
// (pymomentum/tensor_ik/tensor_ik.cpp:129-141).
class BatchedSkeletonSolverFunction {
 public:
  BatchedSkeletonSolverFunction(
      const DeviceCharacter& character,
      size_t batch,
      const std::vector<size_t>& positionParents,
      const std::vector<size_t>& orientationParents)
      : character_(character), batch_(batch), kp_(positionParents.size()), ko_(orientationParents.size()) {
    std::vector<int32_t> pp(positionParents.begin(), positionParents.end());
    std::vector<int32_t> op(orientationParents.begin(), orientationParents.end());
    mmx_problem* h = nullptr;
    check(mmx_problem_create(
        character.handle(), int32_t(batch), int32_t(kp_), pp.data(), int32_t(ko_), op.data(), &h));
    handle_.reset(h, [](mmx_problem* p) { mmx_problem_destroy(p); });
    posOffset_.assign(batch * kp_ * 3, 0.f);
    posTarget_.assign(batch * kp_ * 3, 0.f);
    posWeight_.assign(batch * kp_, 1.f);
    oriOffset_.assign(batch * ko_ * 4, 0.f);
    oriTarget_.assign(batch * ko_ * 4, 0.f);
    for (size_t i = 0; i < batch * ko_; ++i) {
      oriOffset_[4 * i + 3] = 1.f;
      oriTarget_[4 * i + 3] = 1.f;
    }
    oriWeight_.assign(batch * ko_, 1.f);
    posParent_.resize(batch * kp_);
    oriParent_.resize(batch * ko_);
    for (size_t b = 0; b < batch; ++b) {
      std::copy(pp.begin(), pp.end(), posParent_.begin() + b * kp_);
      std::copy(op.begin(), op.end(), oriParent_.begin() + b * ko_);
    }
    sharedPos_ = pp;
    sharedOri_ = op;
  }
  BatchedSkeletonSolverFunction(const BatchedSkeletonSolverFunction&) = delete; // like the reference (:29-32)
  BatchedSkeletonSolverFunction& operator=(const BatchedSkeletonSolverFunction&) = delete;

  size_t getNumParameters() const {
    return character_.numParameters();
  }
  size_t batchSize() const {
    return batch_;
  }
  // One Character per batch element, all of the topology of the DeviceCharacter (same parents and
  // parameter transform; translationOffset / preRotation differ, e.g. per-subject bone lengths).  An
  // empty list goes back to the shared character.
  void setCharacters(const std::vector<const Character*>& characters) {
    if (characters.empty()) {
      check(mmx_problem_set_instance_rig(handle_.get(), nullptr, nullptr, MMX_MEM_HOST, nullptr));
      return;
    }
    const size_t J = character_.numJoints();
    if (characters.size() != batch_) {
      throw std::runtime_error("momentum_amd: one character per batch element expected");
    }
    std::vector<float> off(batch_ * J * 3), pre(batch_ * J * 4);
    for (size_t b = 0; b < batch_; ++b) {
      const Character& c = *characters[b];
      if (c.skeleton.joints.size() != J || c.parameterTransform.numAllModelParameters() != character_.numParameters()) {
        throw std::runtime_error("momentum_amd: per-element characters must share the topology of the device character");
      }
      for (size_t j = 0; j < J; ++j) {
        const Joint& jt = c.skeleton.joints[j];
        const int32_t par = jt.parent == kInvalidIndex ? MMX_INVALID_PARENT : int32_t(jt.parent);
        if (par != character_.parentOf(j)) {
          throw std::runtime_error("momentum_amd: per-element characters must share the topology of the device character");
        }
        for (int k = 0; k < 3; ++k) {
          off[(b * J + j) * 3 + k] = jt.translationOffset[k];
        }
        for (int k = 0; k < 4; ++k) {
          pre[(b * J + j) * 4 + k] = jt.preRotation[k];
        }
      }
    }
    check(mmx_problem_set_instance_rig(handle_.get(), off.data(), pre.data(), MMX_MEM_HOST, nullptr));
  }
  // PositionErrorFunction::setConstraints of batch element b (ConstraintData::parent per constraint)
  void setPositionConstraints(size_t b, const std::vector<PositionData>& c) {
    if (b >= batch_ || c.size() != kp_) {
      throw std::runtime_error("momentum_amd: position constraint count / batch index mismatch");
    }
    for (size_t i = 0; i < kp_; ++i) {
      posParent_[b * kp_ + i] = int32_t(c[i].parent);
      for (int k = 0; k < 3; ++k) {
        posOffset_[(b * kp_ + i) * 3 + k] = c[i].offset[k];
        posTarget_[(b * kp_ + i) * 3 + k] = c[i].target[k];
      }
      posWeight_[b * kp_ + i] = c[i].weight;
    }
    dirty_ = true;
  }
  void setOrientationConstraints(size_t b, const std::vector<OrientationData>& c) {
    if (b >= batch_ || c.size() != ko_) {
      throw std::runtime_error("momentum_amd: orientation constraint count / batch index mismatch");
    }
    for (size_t i = 0; i < ko_; ++i) {
      oriParent_[b * ko_ + i] = int32_t(c[i].parent);
      for (int k = 0; k < 4; ++k) {
        oriOffset_[(b * ko_ + i) * 4 + k] = c[i].offset[k];
        oriTarget_[(b * ko_ + i) * 4 + k] = c[i].target[k];
      }
      oriWeight_[b * ko_ + i] = c[i].weight;
    }
    dirty_ = true;
  }
  void setWeights(float positionWeight, float orientationWeight) { // SkeletonErrorFunction::setWeight
    wPos_ = positionWeight;
    wOri_ = orientationWeight;
    dirty_ = true;
  }
  // Per-element error-function weights: errorFunctionWeights[iBatch][weightsMap[iErr]] of solveTensorIKProblem
  // (pymomentum/tensor_ik/tensor_ik.cpp:100-101,137-138; every error function of element iBatch gets setWeight(entry),
  // tensor_ik_utility.cpp:162-177).  weights: [batch][columns] row-major, columns = position, orientation, limits,
  // model parameters, joint block 0, 1, ... (mmx_constraint_data::function_weights); an empty vector removes them.
  void setErrorFunctionWeights(const std::vector<float>& weights, size_t columns) {
    if (!weights.empty() && (columns == 0 || weights.size() != batch_ * columns)) {
      throw std::runtime_error("momentum_amd: error-function weights must be [batch][columns]");
    }
    fnWeights_ = weights;
    fnCols_ = weights.empty() ? 0 : columns;
    dirty_ = true;
  }
  // LimitErrorFunctionT::setLimits (limit_error_function.h:88) for every element, with its weight_
  void setLimits(const ParameterLimits& limits, float weight = 1.f) {
    limits_.clear();
    for (const ParameterLimit& l : limits) {
      mmx_parameter_limit m{};
      m.type = int32_t(l.type);
      m.index0 = int32_t(l.index0);
      m.index1 = int32_t(l.index1);
      m.weight = l.weight;
      for (int k = 0; k < 4; ++k) {
        m.v[k] = l.values[size_t(k)];
      }
      limits_.push_back(m);
    }
    wLimit_ = weight;
    dirty_ = true;
  }
  // ModelParametersErrorFunctionT::setTargetParameters (model_parameters_error_function.h:48-51) of element b
  void setTargetParameters(size_t b, const std::vector<float>& params, const std::vector<float>& weights, float weight = 1.f) {
    const size_t P = getNumParameters();
    if (b >= batch_ || params.size() != P || weights.size() != P) {
      throw std::runtime_error("momentum_amd: target parameter count / batch index mismatch");
    }
    if (mpTarget_.empty()) {
      mpTarget_.assign(batch_ * P, 0.f);
      mpWeights_.assign(batch_ * P, 0.f);
    }
    std::copy(params.begin(), params.end(), mpTarget_.begin() + b * P);
    std::copy(weights.begin(), weights.end(), mpWeights_.begin() + b * P);
    wModel_ = weight;
    dirty_ = true;
  }
  // GeneralizedLoss(alpha, c) of the position / orientation blocks: the lossAlpha / lossC constructor
  // arguments of PositionErrorFunctionT / OrientationErrorFunctionT (position_error_function.h:41-48)
  void setLoss(float positionAlpha, float positionC, float orientationAlpha, float orientationC) {
    lossPos_[0] = positionAlpha, lossPos_[1] = positionC;
    lossOri_[0] = orientationAlpha, lossOri_[1] = orientationC;
    dirty_ = true;
  }
  // SkeletonSolverFunction::addErrorFunction for one of the further joint error functions
  // (Plane / Aim / FixedAxis / Normal / Projection / Distance); parents are shared by the batch.  Returns the block's index.
  size_t addJointErrorFunction(JointErrorFunctionType type, const std::vector<size_t>& parents, float lossAlpha = 2.f, float lossC = 1.f) {
    if (type == JointErrorFunctionType::JointToJointDistance) {
      throw std::runtime_error("momentum_amd: a joint-to-joint distance function takes two parent lists (addJointToJointDistanceErrorFunction)");
    }
    return addBlock(type, parents, {}, lossAlpha, lossC);
  }
  // JointToJointDistanceErrorFunction: constraint i ties a point of joints1[i] to a point of joints2[i] (shared by the batch;
  // the two may coincide or lie on one chain).  L2 loss only.
  size_t addJointToJointDistanceErrorFunction(const std::vector<size_t>& joints1, const std::vector<size_t>& joints2) {
    if (joints1.size() != joints2.size()) {
      throw std::runtime_error("momentum_amd: joint-to-joint distance function with parent lists of different length");
    }
    return addBlock(JointErrorFunctionType::JointToJointDistance, joints1, joints2, 2.f, 1.f);
  }
  // ProjectionErrorFunction's nearClip (constraints whose depth falls below it are skipped)
  void setNearClip(size_t block, float nearClip) {
    blockAt(block).nearClip = nearClip;
    dirty_ = true;
  }
  void setWeight(size_t block, float weight) { // SkeletonErrorFunction::setWeight of that error function
    blockAt(block).fw = weight;
    dirty_ = true;
  }
  void setConstraints(size_t block, size_t b, const std::vector<PlaneData>& c) {
    Block& k = expect(block, b, c.size(), MMX_JC_PLANE, MMX_JC_HALF_PLANE);
    for (size_t i = 0; i < c.size(); ++i) {
      put(k, b, i, c[i].offset.data(), nullptr, c[i].normal.data(), c[i].d, c[i].weight);
    }
  }
  void setConstraints(size_t block, size_t b, const std::vector<AimData>& c) {
    Block& k = expect(block, b, c.size(), MMX_JC_AIM_DIST, MMX_JC_AIM_DIR);
    for (size_t i = 0; i < c.size(); ++i) {
      put(k, b, i, c[i].localPoint.data(), c[i].localDir.data(), c[i].globalTarget.data(), 0.f, c[i].weight);
    }
  }
  void setConstraints(size_t block, size_t b, const std::vector<FixedAxisData>& c) {
    Block& k = expect(block, b, c.size(), MMX_JC_FIXED_AXIS_DIFF, MMX_JC_FIXED_AXIS_ANGLE);
    for (size_t i = 0; i < c.size(); ++i) {
      put(k, b, i, nullptr, c[i].localAxis.data(), c[i].globalAxis.data(), 0.f, c[i].weight);
    }
  }
  void setConstraints(size_t block, size_t b, const std::vector<NormalData>& c) {
    Block& k = expect(block, b, c.size(), MMX_JC_NORMAL, MMX_JC_NORMAL);
    for (size_t i = 0; i < c.size(); ++i) {
      put(k, b, i, c[i].localPoint.data(), c[i].localNormal.data(), c[i].globalPoint.data(), 0.f, c[i].weight);
    }
  }
  void setConstraints(size_t block, size_t b, const std::vector<ProjectionData>& c) {
    Block& k = expect(block, b, c.size(), MMX_JC_PROJECTION, MMX_JC_PROJECTION);
    for (size_t i = 0; i < c.size(); ++i) {
      const float uv[3] = {c[i].target[0], c[i].target[1], 0.f};
      put(k, b, i, c[i].offset.data(), nullptr, uv, 0.f, c[i].weight);
      std::copy(c[i].projection.begin(), c[i].projection.end(), k.projection.begin() + 12 * (b * k.parent.size() + i));
    }
  }
  void setConstraints(size_t block, size_t b, const std::vector<DistanceData>& c) {
    Block& k = expect(block, b, c.size(), MMX_JC_DISTANCE, MMX_JC_DISTANCE);
    for (size_t i = 0; i < c.size(); ++i) {
      put(k, b, i, c[i].offset.data(), nullptr, c[i].origin.data(), c[i].target, c[i].weight);
    }
  }
  // (the joints of the data must be the lists the function was added with: parents are shared by the batch)
  void setConstraints(size_t block, size_t b, const std::vector<JointToJointDistanceData>& c) {
    Block& k = expect(block, b, c.size(), MMX_JC_JOINT_TO_JOINT_DISTANCE, MMX_JC_JOINT_TO_JOINT_DISTANCE);
    const float none[3] = {0.f, 0.f, 0.f};
    for (size_t i = 0; i < c.size(); ++i) {
      if (int32_t(c[i].joint1) != k.parent[i] || int32_t(c[i].joint2) != k.parentB[i]) {
        throw std::runtime_error("momentum_amd: joint-to-joint distance data names other joints than its error function");
      }
      put(k, b, i, c[i].offset1.data(), c[i].offset2.data(), none, c[i].targetDistance, c[i].weight);
    }
  }
  void setEnabledParameters(const ParameterSet& ps) {
    std::vector<uint8_t> e(character_.numParameters(), 0);
    for (size_t i = 0; i < e.size() && i < ps.size(); ++i) {
      e[i] = ps[i] ? 1 : 0;
    }
    check(mmx_problem_set_enabled(handle_.get(), e.data()));
    numEnabled_ = size_t(std::count(e.begin(), e.end(), uint8_t(1)));
    enabledSet_ = true;
  }
  // the enabled parameters: the size n of the systems mmx_eval_normal_equations and DeviceSkin::normalEquations return
  size_t numEnabledParameters() const {
    return enabledSet_ ? numEnabled_ : character_.numParameters();
  }
  // uploads the constraint payload if it changed
  void sync() {
    if (!dirty_) {
      return;
    }
    mmx_constraint_data d{};
    d.pos_offset = posOffset_.data();
    d.pos_target = posTarget_.data();
    d.pos_weight = posWeight_.data();
    d.ori_offset = oriOffset_.data();
    d.ori_target = oriTarget_.data();
    d.ori_weight = oriWeight_.data();
    d.pos_function_weight = wPos_;
    d.ori_function_weight = wOri_;
    d.memory = MMX_MEM_HOST;
    d.num_limits = int32_t(limits_.size());
    d.limits = limits_.empty() ? nullptr : limits_.data();
    d.limit_function_weight = wLimit_;
    d.model_target = mpTarget_.empty() ? nullptr : mpTarget_.data();
    d.model_weights = mpWeights_.empty() ? nullptr : mpWeights_.data();
    d.model_function_weight = wModel_;
    d.pos_loss_alpha = lossPos_[0], d.pos_loss_c = lossPos_[1];
    d.ori_loss_alpha = lossOri_[0], d.ori_loss_c = lossOri_[1];
    std::vector<mmx_joint_constraint_block> jb(blocks_.size());
    std::vector<std::vector<int32_t>> pairParents(blocks_.size()); // [joints A | joints B] of the pair blocks
    for (size_t i = 0; i < blocks_.size(); ++i) {
      const Block& k = blocks_[i];
      jb[i].type = k.type;
      jb[i].count = int32_t(k.parent.size());
      jb[i].parent = k.parent.data();
      if (k.type == MMX_JC_JOINT_TO_JOINT_DISTANCE) {
        pairParents[i] = k.parent;
        pairParents[i].insert(pairParents[i].end(), k.parentB.begin(), k.parentB.end());
        jb[i].parent = pairParents[i].data();
      }
      jb[i].projection = k.type == MMX_JC_PROJECTION ? k.projection.data() : nullptr;
      jb[i].near_clip = k.nearClip;
      jb[i].local_point = k.localPoint.data();
      jb[i].local_dir = k.localDir.data();
      jb[i].global = k.global.data();
      jb[i].plane_d = k.planeD.data();
      jb[i].weight = k.weight.data();
      jb[i].function_weight = k.fw;
      jb[i].loss_alpha = k.loss[0], jb[i].loss_c = k.loss[1];
    }
    d.num_joint_blocks = int32_t(jb.size());
    d.joint_blocks = jb.empty() ? nullptr : jb.data();
    d.function_weights = fnWeights_.empty() ? nullptr : fnWeights_.data();
    d.num_function_weights = int32_t(fnCols_);
    check(mmx_problem_set_constraints_sized(handle_.get(), &d, sizeof(d), nullptr));
    // per-element parent lists only when some element departs from the constructor's lists
    auto departs = [&](const std::vector<int32_t>& all, const std::vector<int32_t>& shared) {
      for (size_t b = 0; b < batch_; ++b) {
        if (!std::equal(shared.begin(), shared.end(), all.begin() + b * shared.size())) {
          return true;
        }
      }
      return false;
    };
    const bool ip = departs(posParent_, sharedPos_), io = departs(oriParent_, sharedOri_);
    if (ip || io || instanceParents_) {
      check(mmx_problem_set_instance_parents(handle_.get(), ip ? posParent_.data() : nullptr, io ? oriParent_.data() : nullptr, MMX_MEM_HOST, nullptr));
      instanceParents_ = ip || io;
    }
    dirty_ = false;
  }
  // SolverFunctionT::getJacobian for every element: column-major M x P per element, residual M
  void getJacobian(const std::vector<float>& parameters, std::vector<float>& jacobian, std::vector<float>& residual, std::vector<double>& error) {
    sync();
    const size_t M = size_t(mmx_problem_num_rows(handle_.get())), P = getNumParameters();
    if (parameters.size() != batch_ * P) {
      throw std::runtime_error("momentum_amd: parameters.size() != batch * numParameters"); // solver.cpp:77
    }
    jacobian.resize(batch_ * M * P);
    residual.resize(batch_ * M);
    error.resize(batch_);
    check(mmx_eval_jacobian_host(handle_.get(), parameters.data(), jacobian.data(), residual.data(), error.data(), MMX_LAYOUT_COL_MAJOR));
  }
  // SolverFunctionT::getGradient for every element without a Jacobian (mmx_eval_gradient): gradient P per element (2 J^T r,
  // exact zeros for disabled parameters), and the error.  Throws for problems outside the matrix-free kernel's scope (further
  // joint error functions, ellipsoid limits, per-element constraint parents): there is no fallback through getJacobian.
  void getGradient(const std::vector<float>& parameters, std::vector<float>& gradient, std::vector<double>& error) {
    sync();
    const size_t P = getNumParameters();
    if (parameters.size() != batch_ * P) {
      throw std::runtime_error("momentum_amd: parameters.size() != batch * numParameters"); // solver.cpp:77
    }
    gradient.resize(batch_ * P);
    error.resize(batch_);
    check(mmx_eval_gradient_host(handle_.get(), parameters.data(), gradient.data(), error.data()));
  }
  mmx_problem* handle() const {
    return handle_.get();
  }
  const DeviceCharacter& character() const {
    return character_;
  }

 private:
  struct Block {
    int32_t type = 0;
    std::vector<int32_t> parent;
    std::vector<int32_t> parentB; // JointToJointDistance: the second joint of every constraint
    std::vector<float> localPoint, localDir, global, planeD, weight;
    std::vector<float> projection; // Projection: [batch][count][12]
    float nearClip = 1.f;
    float fw = 1.f;
    float loss[2] = {2.f, 1.f};
  };
  size_t addBlock(JointErrorFunctionType type, const std::vector<size_t>& parents, const std::vector<size_t>& parentsB, float lossAlpha, float lossC) {
    if (blocks_.size() >= MMX_MAX_JOINT_BLOCKS) {
      throw std::runtime_error("momentum_amd: too many joint error functions");
    }
    Block k;
    k.type = int32_t(type);
    k.parent.assign(parents.begin(), parents.end());
    k.parentB.assign(parentsB.begin(), parentsB.end());
    const size_t cnt = batch_ * parents.size();
    if (type == JointErrorFunctionType::Projection) {
      k.projection.assign(12 * cnt, 0.f);
    }
    k.localPoint.assign(3 * cnt, 0.f);
    k.localDir.assign(3 * cnt, 0.f);
    k.global.assign(3 * cnt, 0.f);
    k.planeD.assign(cnt, 0.f);
    k.weight.assign(cnt, 0.f); // constraints not set yet carry weight 0 (skipped, joint_error_function-inl.h:197-199)
    k.loss[0] = lossAlpha, k.loss[1] = lossC;
    blocks_.push_back(std::move(k));
    dirty_ = true;
    return blocks_.size() - 1;
  }
  Block& blockAt(size_t block) {
    if (block >= blocks_.size()) {
      throw std::runtime_error("momentum_amd: joint error function index out of range");
    }
    return blocks_[block];
  }
  Block& expect(size_t block, size_t b, size_t count, int32_t typeLo, int32_t typeHi) {
    Block& k = blockAt(block);
    if (b >= batch_ || count != k.parent.size() || k.type < typeLo || k.type > typeHi) {
      throw std::runtime_error("momentum_amd: constraint data does not match the joint error function (type / count / batch index)");
    }
    dirty_ = true;
    return k;
  }
  void put(Block& k, size_t b, size_t i, const float* lp, const float* ld, const float* gl, float d, float w) {
    const size_t c = b * k.parent.size() + i;
    for (int q = 0; q < 3; ++q) {
      k.localPoint[3 * c + q] = lp != nullptr ? lp[q] : 0.f;
      k.localDir[3 * c + q] = ld != nullptr ? ld[q] : 0.f;
      k.global[3 * c + q] = gl[q];
    }
    k.planeD[c] = d;
    k.weight[c] = w;
  }
  std::vector<Block> blocks_;
  const DeviceCharacter& character_; // non-owning, like the reference (:87-88)
  size_t batch_, kp_, ko_;
  std::shared_ptr<mmx_problem> handle_;
  std::vector<float> posOffset_, posTarget_, posWeight_, oriOffset_, oriTarget_, oriWeight_;
  std::vector<int32_t> posParent_, oriParent_, sharedPos_, sharedOri_; // [batch * K] per element ; the constructor's lists
  bool instanceParents_ = false;
  std::vector<mmx_parameter_limit> limits_;
  std::vector<float> mpTarget_, mpWeights_;
  float wPos_ = 1.f, wOri_ = 1.f, wLimit_ = 1.f, wModel_ = 1.f;
  std::vector<float> fnWeights_; // [batch][fnCols_] per-element error-function weights, or empty
  size_t fnCols_ = 0;
  float lossPos_[2] = {2.f, 1.f}, lossOri_[2] = {2.f, 1.f};
  bool dirty_ = true;
  size_t numEnabled_ = 0;
  bool enabledSet_ = false;
};

// GaussNewtonSolverT<float> for every element of the batch at once.
// TransformT<float> (momentum/math/transform.h:36-42): p -> translation + rotation * (scale * p)
struct Transform {
  Vector3f translation{0.f, 0.f, 0.f};
  Quaternionf rotation{0.f, 0.f, 0.f, 1.f}; // (x, y, z, w)
  float scale = 1.f;
  Vector3f transformPoint(const Vector3f& p) const { // transform.h:193 (Eigen's quaternion * vector: v + w uv + qv x uv, uv = 2 qv x v)
    const float x = scale * p[0], y = scale * p[1], z = scale * p[2];
    const float qx = rotation[0], qy = rotation[1], qz = rotation[2], qw = rotation[3];
    const float ux = 2.f * (qy * z - qz * y), uy = 2.f * (qz * x - qx * z), uz = 2.f * (qx * y - qy * x);
    return Vector3f{
        translation[0] + x + qw * ux + (qy * uz - qz * uy),
        translation[1] + y + qw * uy + (qz * ux - qx * uz),
        translation[2] + z + qw * uz + (qx * uy - qy * ux)};
  }
};
// the world-space part of JointStateT<float> (momentum/character/joint_state.h:50-74)
struct JointState {
  Transform transform;
  const Vector3f& translation() const {
    return transform.translation;
  }
  const Quaternionf& rotation() const {
    return transform.rotation;
  }
  float scale() const {
    return transform.scale;
  }
};
// SkeletonStateT<float> (momentum/character/skeleton_state.h:45): jointState[j] of one character
struct SkeletonState {
  std::vector<JointState> jointState;
};
// SkeletonStateT<float>(parameterTransform.apply(modelParameters), skeleton) for every batch element
// (skeleton_state.cpp:22-28,87-121; the forward pass only, call stack SURVEY 3.3): element b is evaluated on ITS
// character when the function carries per-element characters.  modelParameters: [batch][numParameters].
class BatchedSkeletonState {
 public:
  BatchedSkeletonState() = default;
  BatchedSkeletonState(BatchedSkeletonSolverFunction& function, const std::vector<float>& modelParameters) {
    set(function, modelParameters);
  }
  void set(BatchedSkeletonSolverFunction& function, const std::vector<float>& modelParameters) {
    function.sync();
    const size_t B = function.batchSize(), P = function.getNumParameters();
    if (modelParameters.size() != B * P) {
      throw std::runtime_error("momentum_amd: parameters.size() != batch * numParameters"); // parameter_transform.cpp:112-121
    }
    const size_t J = size_t(mmx_rig_num_joints(function.character().handle()));
    std::vector<float> st(B * J * 8);
    check(mmx_eval_skeleton_state_host(function.handle(), modelParameters.data(), st.data()));
    states_.assign(B, SkeletonState{});
    for (size_t b = 0; b < B; ++b) {
      states_[b].jointState.resize(J);
      for (size_t j = 0; j < J; ++j) {
        const float* w = st.data() + (b * J + j) * 8;
        Transform& t = states_[b].jointState[j].transform;
        t.translation = Vector3f{w[0], w[1], w[2]};
        t.rotation = Quaternionf{w[3], w[4], w[5], w[6]};
        t.scale = w[7];
      }
    }
  }
  // The backward pass of set(): with stateGradient [batch][numJoints][8] = dL/d(tx,ty,tz, qx,qy,qz,qw, s) of every joint's
  // world transform at modelParameters, returns dL/dmodelParameters [batch * numParameters] (mmx_eval_skeleton_state_backward:
  // through the skeleton tree, no state Jacobian).  The quaternion part is applied to the rotation as set() returns it.
  static std::vector<float> backward(
      BatchedSkeletonSolverFunction& function, const std::vector<float>& modelParameters, const std::vector<float>& stateGradient) {
    function.sync();
    const size_t B = function.batchSize(), P = function.getNumParameters();
    if (modelParameters.size() != B * P) {
      throw std::runtime_error("momentum_amd: parameters.size() != batch * numParameters");
    }
    const size_t J = size_t(mmx_rig_num_joints(function.character().handle()));
    if (stateGradient.size() != B * J * 8) {
      throw std::runtime_error("momentum_amd: stateGradient.size() != batch * numJoints * 8");
    }
    std::vector<float> grad(B * P);
    check(mmx_eval_skeleton_state_backward_host(function.handle(), modelParameters.data(), stateGradient.data(), grad.data()));
    return grad;
  }
  size_t batchSize() const {
    return states_.size();
  }
  const SkeletonState& operator[](size_t b) const {
    return states_.at(b);
  }

 private:
  std::vector<SkeletonState> states_;
};

// Vertex constraints on a skinned mesh (DeviceSkin::normalEquations; momentum's vertex error function, Position and Plane types):
// per batch element `count` constraints, each a mesh vertex (corners = 1) or a point of a triangle (corners = 3: the
// triangle's vertices and barycentric weights, what DeviceMesh::closestPoints returns), pulled to `target` -- by all three
// coordinates, or with `normal` given along that normal only (point-to-plane; the normal is used as given).
struct VertexConstraints {
  size_t corners = 1; // 1 or 3
  float functionWeight = 1.f;
  std::vector<int32_t> vertex; // [batch][count][corners]; empty with corners = 1: constraint c is vertex c
  std::vector<float> barycentric; // [batch][count][3] with corners = 3
  std::vector<float> target; // [batch][count][3]
  std::vector<float> normal; // [batch][count][3]: plane constraints; empty: position constraints
  std::vector<float> weight; // [batch][count]; empty: 1.  A weight that is not > 0 or a vertex outside [0, V) skips the constraint
  std::vector<float> restPositions; // [batch][V][3] per-element rest vertices; empty: the skin's own
};
// H = J^T J [batch][n][n] (full, symmetric), g = J^T r [batch][n] and the error [batch] over the n enabled parameters, in the
// layout of mmx_eval_normal_equations: a Gauss-Newton step is parameters[enabled] -= (H + lambda I)^-1 g
struct VertexNormalEquations {
  size_t n = 0;
  std::vector<float> jtj, jtr;
  std::vector<double> error;
};

// Linear-blend skinning on a device character (mmx_skin): momentum's SkinWeights (index / weight [V][K], K <= 8),
// Character::inverseBindPose as 3 x 4 row-major affines [J][12] (empty = identity) and the mesh's rest vertices [V][3].
// skinPoints: skeleton state [batch][numJoints][8] = (tx,ty,tz, qx,qy,qz,qw, s) -> posed vertices [batch][V][3] (applySSD for
// every batch element); skinPointsBackward: its vector-Jacobian product.  restPositions: empty (the skin's own) or per-element
// rest vertices [batch][V][3].  The host forms copy in, run, copy out and synchronise; the device forms take device pointers
// and a hipStream_t (as void*) and only enqueue kernels.  The skin shares the character's rig handle and keeps it alive.
class DeviceSkin {
 public:
  struct Gradients {
    std::vector<float> state; // [batch][numJoints][8]
    std::vector<float> restPositions; // [batch][V][3], empty unless asked for
  };
  DeviceSkin(
      const DeviceCharacter& character, size_t maxInfluences, const std::vector<int32_t>& joint, const std::vector<float>& weight,
      const std::vector<float>& inverseBind, const std::vector<float>& restPositions)
      : character_(character), numVertices_(restPositions.size() / 3) {
    if (maxInfluences == 0 || restPositions.size() % 3 != 0 || joint.size() != numVertices_ * maxInfluences || weight.size() != joint.size()) {
      throw std::runtime_error("momentum_amd: skin arrays must be [V][K] (joint, weight) and [V][3] (rest positions)");
    }
    if (!inverseBind.empty() && inverseBind.size() != character.numJoints() * 12) {
      throw std::runtime_error("momentum_amd: inverseBind.size() != numJoints * 12");
    }
    mmx_skin_desc d{};
    d.num_vertices = int32_t(numVertices_);
    d.max_influences = int32_t(maxInfluences);
    d.joint = joint.data();
    d.weight = weight.data();
    d.inverse_bind = inverseBind.empty() ? nullptr : inverseBind.data();
    d.rest_positions = restPositions.data();
    mmx_skin* h = nullptr;
    check(mmx_skin_create(character.handle(), &d, &h));
    handle_.reset(h, [](mmx_skin* p) { mmx_skin_destroy(p); });
  }
  mmx_skin* handle() const {
    return handle_.get();
  }
  size_t numVertices() const {
    return numVertices_;
  }
  std::vector<float> skinPoints(size_t batch, const std::vector<float>& state, const std::vector<float>& restPositions = {}) const {
    checkSizes(batch, state, restPositions);
    std::vector<float> out(batch * numVertices_ * 3);
    check(mmx_skin_points_host(handle_.get(), int32_t(batch), state.data(), restPositions.empty() ? nullptr : restPositions.data(), out.data()));
    return out;
  }
  Gradients skinPointsBackward(
      size_t batch, const std::vector<float>& state, const std::vector<float>& vertexGradient, const std::vector<float>& restPositions = {},
      bool wantRestGradient = false) const {
    checkSizes(batch, state, restPositions);
    if (vertexGradient.size() != batch * numVertices_ * 3) {
      throw std::runtime_error("momentum_amd: vertexGradient.size() != batch * numVertices * 3");
    }
    Gradients g;
    g.state.resize(state.size());
    g.restPositions.resize(wantRestGradient ? vertexGradient.size() : 0);
    check(mmx_skin_points_backward_host(
        handle_.get(), int32_t(batch), state.data(), restPositions.empty() ? nullptr : restPositions.data(), vertexGradient.data(), g.state.data(),
        wantRestGradient ? g.restPositions.data() : nullptr));
    return g;
  }
  // device forms: every pointer is device memory of the character's device; restPositions / restGradient may be null
  void skinPoints(size_t batch, const float* state, const float* restPositions, float* out, void* stream) const {
    check(mmx_skin_points(handle_.get(), int32_t(batch), state, restPositions, out, stream));
  }
  void skinPointsBackward(
      size_t batch, const float* state, const float* restPositions, const float* vertexGradient, float* stateGradient, float* restGradient,
      void* stream) const {
    check(mmx_skin_points_backward(handle_.get(), int32_t(batch), state, restPositions, vertexGradient, stateGradient, restGradient, stream));
  }
  // The Gauss-Newton terms of vertex constraints on this skin at modelParameters [batch][numParameters], over the function's
  // enabled parameters (mmx_skin_normal_equations: one kernel; nothing is solved and the function's own constraints are not
  // read).  `function` must be on the skin's character.  Throws for more than MMX_SKIN_NE_MAX_SOLVED enabled parameters.
  VertexNormalEquations normalEquations(
      const BatchedSkeletonSolverFunction& function, const std::vector<float>& modelParameters, const VertexConstraints& c) const {
    return normalEquationsHost(function, modelParameters, c, -1);
  }
  // ... with every instance's tiles divided over `parts` workgroups (mmx_skin_normal_equations_split_host: 1..
  // MMX_SKIN_NE_MAX_PARTS, or 0 for the library's plan; for few instances against a dense mesh).  parts = 1 gives the bits of
  // the form above; an instance's bits depend on its inputs and min(parts, tiles) only.
  VertexNormalEquations normalEquations(
      const BatchedSkeletonSolverFunction& function, const std::vector<float>& modelParameters, const VertexConstraints& c, int32_t parts) const {
    if (parts < 0) {
      throw std::runtime_error("momentum_amd: parts must be >= 0");
    }
    return normalEquationsHost(function, modelParameters, c, parts);
  }
  // device form: the descriptor's arrays, modelParameters and the outputs (any of them null, not all) are device memory
  void normalEquations(
      const BatchedSkeletonSolverFunction& function, const mmx_vertex_constraints& deviceArrays, const float* modelParameters, float* jtj,
      float* jtr, double* error, void* stream) const {
    check(mmx_skin_normal_equations(function.handle(), handle_.get(), &deviceArrays, modelParameters, jtj, jtr, error, stream));
  }
  // ... split: `workspace` is device memory of normalEquationsWorkspaceBytes(function, parts) bytes, 16-byte aligned (may be
  // null when the effective parts is 1); two kernels on `stream`
  void normalEquations(
      const BatchedSkeletonSolverFunction& function, const mmx_vertex_constraints& deviceArrays, const float* modelParameters, float* jtj,
      float* jtr, double* error, int32_t parts, void* workspace, int64_t workspaceBytes, void* stream) const {
    check(mmx_skin_normal_equations_split(
        function.handle(), handle_.get(), &deviceArrays, modelParameters, jtj, jtr, error, parts, workspace, workspaceBytes, stream));
  }
  // what parts = 0 resolves to for this function, skin and descriptor (type, count and corners are read, the arrays are not)
  int32_t normalEquationsAutoParts(const BatchedSkeletonSolverFunction& function, const mmx_vertex_constraints& descriptor) const {
    int32_t parts = 0;
    check(mmx_skin_normal_equations_auto_parts(function.handle(), handle_.get(), &descriptor, &parts));
    return parts;
  }
  static int64_t normalEquationsWorkspaceBytes(const BatchedSkeletonSolverFunction& function, int32_t parts) {
    return mmx_skin_normal_equations_workspace_bytes(int32_t(function.batchSize()), int32_t(function.numEnabledParameters()), parts);
  }

 private:
  VertexNormalEquations normalEquationsHost(
      const BatchedSkeletonSolverFunction& function, const std::vector<float>& modelParameters, const VertexConstraints& c, int32_t parts) const {
    const size_t batch = function.batchSize(), count = c.target.size() / (3 * (batch ? batch : 1));
    if (modelParameters.size() != batch * function.getNumParameters()) {
      throw std::runtime_error("momentum_amd: modelParameters.size() != batch * numParameters");
    }
    auto sized = [&](size_t have, size_t per, bool optional) { return (optional && have == 0) || have == batch * count * per; };
    if (count == 0 || c.target.size() != batch * count * 3 || !sized(c.vertex.size(), c.corners, c.corners == 1) ||
        !sized(c.barycentric.size(), 3, c.corners == 1) || !sized(c.normal.size(), 3, true) || !sized(c.weight.size(), 1, true) ||
        (!c.restPositions.empty() && c.restPositions.size() != batch * numVertices_ * 3)) {
      throw std::runtime_error("momentum_amd: vertex constraint arrays must be [batch][count][...] with one count");
    }
    mmx_vertex_constraints d{};
    d.type = c.normal.empty() ? MMX_VC_POSITION : MMX_VC_PLANE;
    d.count = int32_t(count);
    d.corners = int32_t(c.corners);
    d.function_weight = c.functionWeight;
    d.vertex = c.vertex.empty() ? nullptr : c.vertex.data();
    d.barycentric = c.barycentric.empty() ? nullptr : c.barycentric.data();
    d.target = c.target.data();
    d.normal = c.normal.empty() ? nullptr : c.normal.data();
    d.weight = c.weight.empty() ? nullptr : c.weight.data();
    d.rest = c.restPositions.empty() ? nullptr : c.restPositions.data();
    VertexNormalEquations out;
    out.n = function.numEnabledParameters();
    out.jtj.resize(batch * out.n * out.n);
    out.jtr.resize(batch * out.n);
    out.error.resize(batch);
    if (parts < 0) {
      check(mmx_skin_normal_equations_host(function.handle(), handle_.get(), &d, modelParameters.data(), out.jtj.data(), out.jtr.data(), out.error.data()));
    } else {
      check(mmx_skin_normal_equations_split_host(
          function.handle(), handle_.get(), &d, modelParameters.data(), out.jtj.data(), out.jtr.data(), out.error.data(), parts));
    }
    return out;
  }
  void checkSizes(size_t batch, const std::vector<float>& state, const std::vector<float>& restPositions) const {
    if (batch == 0 || state.size() != batch * character_.numJoints() * 8) {
      throw std::runtime_error("momentum_amd: state.size() != batch * numJoints * 8");
    }
    if (!restPositions.empty() && restPositions.size() != batch * numVertices_ * 3) {
      throw std::runtime_error("momentum_amd: restPositions.size() != batch * numVertices * 3");
    }
  }
  DeviceCharacter character_; // (shares the rig handle: keeps it alive)
  std::shared_ptr<mmx_skin> handle_;
  size_t numVertices_ = 0;
};

// Closest points ON a posed mesh (DeviceMesh::closestPoints / findClosestPointsOnMesh below)
struct ClosestPointsOnMeshOptions {
  float maxDist = std::numeric_limits<float>::infinity();
  bool verticesShared = false; // vertices are [V][3], shared by the batch
};
struct ClosestPointsOnMesh {
  std::vector<int32_t> faceIndex; // [batch][numSource], -1 = no eligible triangle
  std::vector<float> barycentric; // [batch][numSource][3] = (w_a, w_b, w_c), zeros where faceIndex is -1
  std::vector<float> points; // [batch][numSource][3], zeros where faceIndex is -1
  std::vector<float> dist2; // [batch][numSource], +inf where faceIndex is -1
};

// Vertex normals on a device mesh (mmx_mesh): momentum's Mesh::updateNormals / pymomentum.geometry.compute_vertex_normals for a
// batch of posed meshes that share their triangles [T][3].  vertexNormals: positions [batch][V][3] -> unit normals
// [batch][V][3], the normalised sum of the face vectors (p_b - p_a) x (p_c - p_a) of a vertex's triangles (area-weighted;
// zeros where the sum is zero, NaN where it is not finite) and, for the backward pass, the unnormalised sums;
// vertexNormalsBackward: its vector-Jacobian product.  The device forms take device pointers of the mesh's device and a
// hipStream_t (as void*) and enqueue one kernel each on the handle the constructor uploaded; the host forms copy in, run, copy
// out and synchronise (the convenience form: they build a handle of their own per call).
class DeviceMesh {
 public:
  struct Normals {
    std::vector<float> normals; // [batch][V][3]
    std::vector<float> sums; // [batch][V][3], what vertexNormalsBackward reads
  };
  DeviceMesh(size_t numVertices, const std::vector<int32_t>& triangles, int device = 0)
      : numVertices_(numVertices), device_(device), triangles_(triangles) {
    if (triangles.empty() || triangles.size() % 3 != 0 || numVertices > size_t(std::numeric_limits<int32_t>::max()) ||
        triangles.size() / 3 > size_t(std::numeric_limits<int32_t>::max())) {
      throw std::runtime_error("momentum_amd: triangles must be [T][3] with T >= 1, and the sizes must fit int32");
    }
    mmx_mesh* h = nullptr;
    check(mmx_mesh_create(int32_t(numVertices), int32_t(triangles.size() / 3), triangles.data(), int32_t(device), &h));
    handle_.reset(h, [](mmx_mesh* p) { mmx_mesh_destroy(p); });
  }
  mmx_mesh* handle() const {
    return handle_.get();
  }
  size_t numVertices() const {
    return numVertices_;
  }
  size_t numTriangles() const {
    return triangles_.size() / 3;
  }
  Normals vertexNormals(size_t batch, const std::vector<float>& positions) const {
    checkSize(batch, positions, "positions");
    Normals r;
    r.normals.resize(positions.size()), r.sums.resize(positions.size());
    check(mmx_vertex_normals_host(
        int32_t(numVertices_), int32_t(numTriangles()), triangles_.data(), int32_t(device_), int32_t(batch), positions.data(), r.normals.data(),
        r.sums.data()));
    return r;
  }
  std::vector<float> vertexNormalsBackward(
      size_t batch, const std::vector<float>& positions, const std::vector<float>& sums, const std::vector<float>& normalGradient) const {
    checkSize(batch, positions, "positions");
    checkSize(batch, sums, "sums");
    checkSize(batch, normalGradient, "normalGradient");
    std::vector<float> out(positions.size());
    check(mmx_vertex_normals_backward_host(
        int32_t(numVertices_), int32_t(numTriangles()), triangles_.data(), int32_t(device_), int32_t(batch), positions.data(), sums.data(),
        normalGradient.data(), out.data()));
    return out;
  }
  // Closest points ON the posed mesh (mmx_closest_points_on_mesh; pymomentum.geometry.find_closest_points_on_mesh, which runs on
  // the CPU): for every source point [batch][numSource][3] the nearest point of the nearest eligible triangle of the same batch
  // element's vertices [batch][V][3] (or [V][3] shared), with its face index and barycentric weights.  A triangle with a
  // repeated vertex or a non-finite vertex is never returned; ties go to the lowest face index.
  ClosestPointsOnMesh closestPoints(
      size_t batch, const std::vector<float>& source, const std::vector<float>& vertices, const ClosestPointsOnMeshOptions& options = {}) const {
    checkSize(options.verticesShared ? 1 : batch, vertices, "vertices");
    if (batch == 0 || batch > size_t(std::numeric_limits<int32_t>::max()) || source.empty() || source.size() % (3 * batch) != 0) {
      throw std::runtime_error("momentum_amd: source must be [batch][numSource][3]");
    }
    const size_t n = source.size() / (3 * batch);
    ClosestPointsOnMesh r;
    r.faceIndex.resize(batch * n), r.barycentric.resize(batch * n * 3), r.points.resize(batch * n * 3), r.dist2.resize(batch * n);
    check(mmx_closest_points_on_mesh_host(
        int32_t(numVertices_), int32_t(numTriangles()), triangles_.data(), int32_t(device_), int32_t(batch), int32_t(n), source.data(),
        vertices.data(), options.verticesShared ? 1 : 0, options.maxDist, r.faceIndex.data(), r.barycentric.data(), r.points.data(),
        r.dist2.data()));
    return r;
  }
  // device forms: every pointer is device memory of the mesh's device; sums may be null in the forward; barycentric, points and
  // dist2 may be null in closestPoints
  void closestPoints(
      size_t batch, size_t numSource, const float* source, const float* vertices, const ClosestPointsOnMeshOptions& options, int32_t* faceIndex,
      float* barycentric, float* points, float* dist2, void* stream) const {
    check(mmx_closest_points_on_mesh(
        handle_.get(), int32_t(batch), int32_t(numSource), source, vertices, options.verticesShared ? 1 : 0, options.maxDist, faceIndex, barycentric,
        points, dist2, stream));
  }
  void vertexNormals(size_t batch, const float* positions, float* normals, float* sums, void* stream) const {
    check(mmx_vertex_normals(handle_.get(), int32_t(batch), positions, normals, sums, stream));
  }
  void vertexNormalsBackward(
      size_t batch, const float* positions, const float* sums, const float* normalGradient, float* positionGradient, void* stream) const {
    check(mmx_vertex_normals_backward(handle_.get(), int32_t(batch), positions, sums, normalGradient, positionGradient, stream));
  }

 private:
  void checkSize(size_t batch, const std::vector<float>& a, const char* what) const {
    if (batch == 0 || batch > size_t(std::numeric_limits<int32_t>::max()) || a.size() != batch * numVertices_ * 3) {
      throw std::runtime_error(std::string("momentum_amd: ") + what + ".size() != batch * numVertices * 3");
    }
  }
  std::shared_ptr<mmx_mesh> handle_;
  size_t numVertices_ = 0;
  int device_ = 0;
  std::vector<int32_t> triangles_; // (the host forms take the mesh itself)
};

// Nearest-point queries (mmx_closest_points; pymomentum.geometry.find_closest_points, which runs on the CPU): for every
// source point [batch][numSource][3] the nearest eligible target point of the same batch element -- targets
// [batch][numTarget][3], or [numTarget][3] shared by the batch.  Eligible: a finite squared distance <= maxDist^2 and, with
// normals (both arrays or neither, laid out like the points, not renormalised), n_s . n_t >= minNormalDot.  Ties go to the
// lowest index.  The device form takes device pointers of the current device and a hipStream_t (as void*) and enqueues one
// kernel: index [batch][numSource] is -1 without an eligible target, dist2 (may be null) is +inf there, points (may be
// null) zeros.  The host form copies in, runs, copies out and synchronises.
struct ClosestPointsOptions {
  float maxDist = std::numeric_limits<float>::infinity();
  float minNormalDot = 0.f; // read only with normals
  bool targetShared = false;
};
inline void findClosestPoints(
    size_t batch, size_t numSource, size_t numTarget, const float* source, const float* target, const float* sourceNormals,
    const float* targetNormals, const ClosestPointsOptions& options, int32_t* index, float* dist2, float* points, void* stream) {
  check(mmx_closest_points(
      int32_t(batch), int32_t(numSource), int32_t(numTarget), source, target, options.targetShared ? 1 : 0, sourceNormals, targetNormals,
      options.maxDist, options.minNormalDot, index, dist2, points, stream));
}
struct ClosestPoints {
  std::vector<int32_t> index; // [batch][numSource], -1 = no eligible target
  std::vector<float> dist2; // [batch][numSource], +inf where index is -1
  std::vector<float> points; // [batch][numSource][3], zeros where index is -1
};
inline ClosestPoints findClosestPoints(
    size_t batch, const std::vector<float>& source, const std::vector<float>& target, const ClosestPointsOptions& options = {},
    const std::vector<float>& sourceNormals = {}, const std::vector<float>& targetNormals = {}) {
  const size_t targetBatch = options.targetShared ? 1 : batch;
  if (batch == 0 || source.empty() || target.empty() || source.size() % (3 * batch) != 0 || target.size() % (3 * targetBatch) != 0) {
    throw std::runtime_error("momentum_amd: source must be [batch][numSource][3] and target [batch][numTarget][3] (or [numTarget][3] when shared)");
  }
  if (sourceNormals.empty() != targetNormals.empty() || (!sourceNormals.empty() && (sourceNormals.size() != source.size() || targetNormals.size() != target.size()))) {
    throw std::runtime_error("momentum_amd: sourceNormals and targetNormals: both or neither, laid out like the points");
  }
  const size_t n = source.size() / (3 * batch), m = target.size() / (3 * targetBatch);
  ClosestPoints r;
  r.index.resize(batch * n);
  r.dist2.resize(batch * n);
  r.points.resize(batch * n * 3);
  check(mmx_closest_points_host(
      int32_t(batch), int32_t(n), int32_t(m), source.data(), target.data(), options.targetShared ? 1 : 0,
      sourceNormals.empty() ? nullptr : sourceNormals.data(), targetNormals.empty() ? nullptr : targetNormals.data(), options.maxDist,
      options.minNormalDot, r.index.data(), r.dist2.data(), r.points.data()));
  return r;
}

// ... and ON a posed mesh: the call shape of pymomentum.geometry.find_closest_points_on_mesh (DeviceMesh::closestPoints)
inline ClosestPointsOnMesh findClosestPointsOnMesh(
    const DeviceMesh& mesh, size_t batch, const std::vector<float>& source, const std::vector<float>& vertices,
    const ClosestPointsOnMeshOptions& options = {}) {
  return mesh.closestPoints(batch, source, vertices, options);
}

class BatchedGaussNewtonSolver {
 public:
  BatchedGaussNewtonSolver(const SolverOptions& options, BatchedSkeletonSolverFunction* function) : fn_(function) {
    setOptions(options);
  }
  virtual ~BatchedGaussNewtonSolver() = default;
  virtual std::string getName() const {
    return "GaussNewton";
  }
  void setOptions(const SolverOptions& options) { // gauss_newton_solver.cpp:37-46
    mmx_gn_options_default(&opt_);
    opt_.min_iterations = int32_t(options.minIterations);
    opt_.max_iterations = int32_t(options.maxIterations);
    opt_.threshold = options.threshold;
    if (const auto* d = dynamic_cast<const GaussNewtonSolverBaseOptions*>(&options)) {
      opt_.regularization = d->regularization;
      opt_.do_line_search = d->doLineSearch ? lineSearchRule() : MMX_LINE_SEARCH_NONE;
    }
    applyDerivedOptions(options, opt_);
    opt_.precision = precision_;
    opt_.precision_bound = precisionBound_;
  }
  void setEnabledParameters(const ParameterSet& ps) {
    fn_->setEnabledParameters(ps);
  }
  // mmx_gn_options::precision (ABI 10) of solve(std::vector<float>&): MMX_PRECISION_F32 (default), MMX_PRECISION_F64 (every
  // element by the double instantiation, float parameters in and out), MMX_PRECISION_AUTO (the elements the single-precision
  // solve marks MMX_SOLVE_PRECISION_SUSPECT are solved again in double); bound <= 0 keeps the default (1e-5).  Kept across
  // setOptions().
  void setPrecision(int32_t precision, float bound = 0.f) {
    precision_ = precision;
    precisionBound_ = bound;
    opt_.precision = precision;
    opt_.precision_bound = bound;
  }
  // parameters [batch * P] in/out; returns the value SolverT::solve returns, per element
  std::vector<double> solve(std::vector<float>& parameters) {
    fn_->sync();
    const size_t B = fn_->batchSize(), P = fn_->getNumParameters();
    if (parameters.size() != B * P) {
      throw std::runtime_error("momentum_amd: parameters.size() != batch * numParameters"); // solver.cpp:77
    }
    std::vector<double> err(B);
    iterations_.assign(B, 0);
    status_.assign(B, 0);
    check(mmx_solve_host(fn_->handle(), &opt_, parameters.data(), err.data(), iterations_.data(), status_.data()));
    return err;
  }
  // Warm-started frame sequences in one launch (mmx_solve_frames; the per-frame loop of marker_tracker.cpp:905-913 for
  // batch / numFrames independent sequences): the function's batch is numFrames x S elements, FRAME-MAJOR -- element f S + s
  // carries the constraints of frame f of sequence s.  parameters [numFrames * S * P]: in, the rows of frame 0 (the later rows
  // are not read); out, every frame's result, frame f solved from the result of frame f - 1.  The one-wavefront route's scope
  // (include/mmx.h); getIterations() / getStatus() per element as after solve.
  std::vector<double> solveFrames(std::vector<float>& parameters, size_t numFrames) {
    fn_->sync();
    const size_t B = fn_->batchSize(), P = fn_->getNumParameters();
    if (parameters.size() != B * P) {
      throw std::runtime_error("momentum_amd: parameters.size() != batch * numParameters"); // solver.cpp:77
    }
    std::vector<double> err(B);
    iterations_.assign(B, 0);
    status_.assign(B, 0);
    check(mmx_solve_frames_host(fn_->handle(), &opt_, int32_t(numFrames), parameters.data(), err.data(), iterations_.data(), status_.data()));
    return err;
  }
  // SolverT<double>::solve with GaussNewtonSolverT<double> for every element (the reference instantiates its
  // solvers for float and double, gauss_newton_solver.cpp:315-316): parameters [batch * P] in double
  std::vector<double> solve(std::vector<double>& parameters) {
    fn_->sync();
    const size_t B = fn_->batchSize(), P = fn_->getNumParameters();
    if (parameters.size() != B * P) {
      throw std::runtime_error("momentum_amd: parameters.size() != batch * numParameters"); // solver.cpp:77
    }
    std::vector<double> err(B);
    iterations_.assign(B, 0);
    status_.assign(B, 0);
    check(mmx_solve_f64_host(fn_->handle(), &opt_, parameters.data(), err.data(), iterations_.data(), status_.data()));
    return err;
  }
  const std::vector<int32_t>& getIterations() const {
    return iterations_;
  }
  const std::vector<int32_t>& getStatus() const {
    return status_;
  }

 protected:
  virtual int32_t lineSearchRule() const { // gauss_newton_solver.cpp:283-313
    return MMX_LINE_SEARCH_GAUSS_NEWTON;
  }
  virtual void applyDerivedOptions(const SolverOptions&, mmx_gn_options&) const {}

 private:
  BatchedSkeletonSolverFunction* fn_; // raw pointer like SolverT::solverFunction_ (solver.h:106)
  mmx_gn_options opt_{};
  int32_t precision_ = MMX_PRECISION_F32;
  float precisionBound_ = 0.f;
  std::vector<int32_t> iterations_, status_;
};

// SubsetGaussNewtonSolverT<float> / GaussNewtonSolverQRT<float> for every element of the batch: the
// regularised normal equations of GaussNewtonSolverT (the QR solver factors [J; sqrt(lambda) I],
// gauss_newton_solver_qr.cpp:75-77, which is the same least-squares problem), with the directional
// line search both share (subset_gauss_newton_solver.cpp:117-142, gauss_newton_solver_qr.cpp:126-149).
class BatchedSubsetGaussNewtonSolver : public BatchedGaussNewtonSolver {
 public:
  BatchedSubsetGaussNewtonSolver(const SolverOptions& options, BatchedSkeletonSolverFunction* function)
      : BatchedGaussNewtonSolver(SolverOptions(options), function) {
    setOptions(options); // the base constructor ran with the base class's rule
  }
  std::string getName() const override {
    return "SubsetGaussNewton";
  }

 protected:
  int32_t lineSearchRule() const override {
    return MMX_LINE_SEARCH_DIRECTIONAL;
  }
};
class BatchedGaussNewtonSolverQR : public BatchedSubsetGaussNewtonSolver {
 public:
  using BatchedSubsetGaussNewtonSolver::BatchedSubsetGaussNewtonSolver;
  std::string getName() const override {
    return "GaussNewtonQR";
  }
};

// TrustRegionQRT<float> (and, through solve(std::vector<double>&), <double>) for every element of the batch
// (trust_region_qr.cpp:52-270): the step rule
// MMX_STEP_TRUST_REGION -- radius, up to ten trust steps per iteration, Newton updates of the damping, gain-ratio
// radius update -- inside the one-launch solve where the problem fits it, on the wide route otherwise
// (larger systems, further joint error functions, ellipsoid limits).
class BatchedTrustRegionQR : public BatchedGaussNewtonSolver {
 public:
  BatchedTrustRegionQR(const SolverOptions& options, BatchedSkeletonSolverFunction* function)
      : BatchedGaussNewtonSolver(SolverOptions(options), function) {
    setOptions(options); // the base constructor ran without this class's hook
  }
  std::string getName() const override {
    return "TrustRegionQR";
  }

 protected:
  void applyDerivedOptions(const SolverOptions& options, mmx_gn_options& o) const override {
    o.step_rule = MMX_STEP_TRUST_REGION;
    o.do_line_search = MMX_LINE_SEARCH_NONE;
    if (const auto* d = dynamic_cast<const TrustRegionQROptions*>(&options)) {
      o.trust_region_radius = d->trustRegionRadius_;
    }
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Single-instance forms under momentum's own names and signatures -- what a per-frame caller holds
// (momentum/marker_tracking/marker_tracker.cpp:905-913: one SkeletonSolverFunction, one solver, solve(parameters) per
// frame): a batch of one element behind momentum/character_solver/skeleton_solver_function.h:21-95 and
// momentum/solver/solver.h:41-106.  (A GPU launch per frame is latency, not throughput: 0.5 ms per solve whatever the
// batch up to ~768 elements; callers with many frames at hand should batch them.)
// ---------------------------------------------------------------------------------------------------------------------
class SkeletonSolverFunction : public BatchedSkeletonSolverFunction {
 public:
  SkeletonSolverFunction(const DeviceCharacter& character, const std::vector<size_t>& positionParents, const std::vector<size_t>& orientationParents)
      : BatchedSkeletonSolverFunction(character, 1, positionParents, orientationParents) {}
  using BatchedSkeletonSolverFunction::setConstraints;
  void setPositionConstraints(const std::vector<PositionData>& c) {
    BatchedSkeletonSolverFunction::setPositionConstraints(0, c);
  }
  void setOrientationConstraints(const std::vector<OrientationData>& c) {
    BatchedSkeletonSolverFunction::setOrientationConstraints(0, c);
  }
  void setTargetParameters(const std::vector<float>& params, const std::vector<float>& weights, float weight = 1.f) {
    BatchedSkeletonSolverFunction::setTargetParameters(0, params, weights, weight);
  }
  template <class Data>
  void setConstraints(size_t block, const std::vector<Data>& c) {
    BatchedSkeletonSolverFunction::setConstraints(block, 0, c);
  }
  // SolverFunctionT::getJacobian (momentum/solver/solver_function.h): Jacobian [rows x P] column-major, residual, returns the error
  double getJacobian(const std::vector<float>& parameters, std::vector<float>& jacobian, std::vector<float>& residual) {
    std::vector<double> e;
    BatchedSkeletonSolverFunction::getJacobian(parameters, jacobian, residual, e);
    return e.at(0);
  }
  // SolverFunctionT::getGradient: gradient [P] without a Jacobian (mmx_eval_gradient), returns the error
  double getGradient(const std::vector<float>& parameters, std::vector<float>& gradient) {
    std::vector<double> e;
    BatchedSkeletonSolverFunction::getGradient(parameters, gradient, e);
    return e.at(0);
  }
  // SolverFunctionT::getError: the same evaluation without keeping the Jacobian
  double getError(const std::vector<float>& parameters) {
    std::vector<float> j, r;
    return getJacobian(parameters, j, r);
  }
};

// SolverT::solve(Eigen::VectorX<T>& params) -> double (momentum/solver/solver.h:62) over the batched solvers: one element
template <class BatchedSolver>
class SingleInstanceSolverT : public BatchedSolver {
 public:
  SingleInstanceSolverT(const SolverOptions& options, SkeletonSolverFunction* function) : BatchedSolver(options, function) {}
  double solve(std::vector<float>& parameters) {
    return BatchedSolver::solve(parameters).at(0);
  }
  double solve(std::vector<double>& parameters) {
    return BatchedSolver::solve(parameters).at(0);
  }
  int32_t iterations() const {
    return this->getIterations().at(0);
  }
  int32_t status() const {
    return this->getStatus().at(0);
  }
};
using GaussNewtonSolver = SingleInstanceSolverT<BatchedGaussNewtonSolver>;
using SubsetGaussNewtonSolver = SingleInstanceSolverT<BatchedSubsetGaussNewtonSolver>;
using GaussNewtonSolverQR = SingleInstanceSolverT<BatchedGaussNewtonSolverQR>;
using TrustRegionQR = SingleInstanceSolverT<BatchedTrustRegionQR>;

} // namespace momentum_amd
