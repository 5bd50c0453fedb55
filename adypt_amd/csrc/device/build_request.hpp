// What every entry that gives a context (or the host) a new tree is asked for, and THE rules for it: the SAH costs of the collapse with their
// defaults, the method, the PLOC radius and the split budget.  Device and host units take defaults and checks from here; the entry points differ only
// in which of the two checks they apply and between which checks of their own (One build request).  No HIP needed.  Not part of the C-ABI.
#pragma once
#include "ploc.hpp"
#include "wide_cut.hpp"
#include "../../../include/adypt_host.h"

namespace adypt {

constexpr int kBuildLinear = 0, kBuildPloc = 1; // `method` of include/adypt_hip.h

struct BuildRequest {
	adypt_bvh_params cfg; // (max_spatial_depth is not looked at: no builder here splits spatially)
	int method;
	int radius;           // counts for kBuildPloc only
	double split_budget;  // 0: no triangle is split
};

// InstanceConfig::BVH's defaults where the caller gives none
inline adypt_bvh_params build_cfg(const adypt_bvh_params *params) { return params ? *params : adypt_bvh_params{0, 0.3f, 1.0f}; }
// the shapes of adypt_rebuild_bvh, _ploc and _ploc_split and of their host twins adypt_bvh_build_linear, _ploc and _ploc_split
inline BuildRequest request_linear(const adypt_bvh_params *params) { return BuildRequest{build_cfg(params), kBuildLinear, 0, 0.0}; }
inline BuildRequest request_ploc(const adypt_bvh_params *params, int radius, double split_budget = 0.0) { return BuildRequest{build_cfg(params), kBuildPloc, radius, split_budget}; }

// Each check: the reason without the caller's name in front, or null.
// The collapse compares sums of these costs times areas against kCutMax: both must be positive and below it (NaN is refused).  `below`: the host's
// adypt_bvh_cost, which only prices a tree, has always taken FLT_MAX itself and passes +inf
inline const char *sah_refused(const adypt_bvh_params &cfg, float below = kCutMax)
{
	const bool ok = cfg.triangle_sah > 0.0f && cfg.triangle_sah < below && cfg.node_sah > 0.0f && cfg.node_sah < below;
	return ok ? nullptr : "the SAH costs must be positive finite numbers";
}
static_assert(kPlocMinRadius == 1 && kPlocMaxRadius == 32, "the text of radius_refused");
inline const char *radius_refused(int radius) { return radius < kPlocMinRadius || radius > kPlocMaxRadius ? "the radius must be in [1, 32]" : nullptr; }
inline const char *budget_refused(double split_budget) { return split_budget >= 0.0 && split_budget <= 1.0 ? nullptr : "the split budget must be in [0, 1]"; } // (NaN is refused)
// in this order: the method is one of the two, the radius where it counts, the budget's range, and no budget without the method that splits
inline const char *method_refused(int method, int radius, double split_budget)
{
	if(method != kBuildLinear && method != kBuildPloc) return "method must be 0 (linear) or 1 (ploc)";
	if(const char *why = method == kBuildPloc ? radius_refused(radius) : nullptr) return why;
	if(const char *why = budget_refused(split_budget)) return why;
	return method == kBuildLinear && split_budget != 0.0 ? "a split budget needs method 1 (ploc)" : nullptr;
}
// both, where an entry has no check of its own between them
inline const char *request_refused(const BuildRequest &q) { const char *why = sah_refused(q.cfg); return why ? why : method_refused(q.method, q.radius, q.split_budget); }

}  // namespace adypt
