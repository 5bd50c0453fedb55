// The limits k_path's path word puts on a pass (path.hpp), free of HIP: frame_plan.hpp decides with them which passes take the one-launch pipeline.
#pragma once
#include <cstdint>

namespace adypt {

constexpr uint32_t kPwBounceShift = 26;          // path word in the table: bits 25..0 path id, 30..26 bounce index (kPwShadow: the ray is the path's sun-visibility query), 31 radiance parked
constexpr uint32_t kPwShadow = 31;               // (so the query needs max_bounce <= 31: frame_plan.hpp keeps the launch-per-bounce pipeline otherwise)
constexpr int64_t kPathMaxPaths = (int64_t)1 << kPwBounceShift; // batches with more paths keep the launch-per-bounce pipeline

}  // namespace adypt
