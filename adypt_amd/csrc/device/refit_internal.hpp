// What build.hip needs of refit.hip: how a triangle record's positions are read, the levels of a tree as the refit keeps them, the launches that turn
// a topology plus triangles into Woop data and node records, and the hand-over of a new tree's levels to the context's refit state.  What pose.hip
// needs of it: the refit around another writer of the records, and the refit-or-rebuild policy around that.  Not part of the C-ABI.
#pragma once
#include "build_request.hpp"
#include "ctx_access.hpp"
#include "resources.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace adypt {

// floats 0..8 of a triangle record (shade.hpp): the three vertices, as woop.hpp, refit.hpp and lbvh.hpp take them
__device__ __forceinline__ void load_positions(const float4 *rec, float p[9])
{
	const float4 a = rec[0], b = rec[1], c = rec[2];
	p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w; p[8] = c.x;
}

// What a refit needs of a tree once it is planned (refit_plan.hpp) or built (build.hip): level l is order[level_begin[l] .. level_begin[l + 1]), the
// nodes in any order inside a level
struct TreeLevels {
	std::vector<int64_t> level_begin; // levels + 1 entries
	Buffer<int32_t> order;            // device: 4 B per node
	Buffer<float4> boxes;             // device: the exact boxes, 2 float4 per node
	Buffer<float4> ref_boxes;         // device: a tree built with split triangles (presplit.hpp) — the box of every reference, 2 float4 each, in the order of
	                                  // tri_indices; empty for every other tree, and dropped by the first adypt_update_triangles (which bounds whole triangles)
	int levels() const { return (int)level_begin.size() - 1; }
};

// k_refit_woop: one thread per reference
hipError_t refit_launch_woop(hipStream_t stream, const float4 *triangles, int tri_float4, const int32_t *tri_indices, int64_t n_refs, float4 *woop);
// k_refit_nodes once per level, deepest first: a level reads the exact boxes that the launches before it on the same stream wrote.  ref_boxes: a leaf
// slot bounds these boxes of its references (2 float4 per reference, in the order of tri_indices) instead of their whole triangles
hipError_t refit_launch_levels(hipStream_t stream, const TreeLevels &tree, uint4 *nodes, const int32_t *tri_indices, const float4 *triangles, int tri_float4, const float4 *ref_boxes = nullptr);
// The context's tree has been replaced: `tree` is taken as the refit's.  A later adypt_update_triangles refits the new topology; the timing of the last
// update is no longer to be read.
void refit_adopt_tree(adypt_ctx *c, TreeLevels &&tree);

// ---- one refit around whoever writes the moved records: adypt_update_triangles' k_refit_scatter, adypt_pose's k_pose (pose.hip) ----
// Before the writer's launches: the context is drained, the plan made (at the first refit of a tree), the timing of the last refit invalidated and the
// first timer mark put on the context's stream.
int refit_begin(adypt_ctx *c);
// Behind the writer's launches on the context's stream, which end the `scatter` stage of adypt_get_refit_timing: a split tree's reference boxes are
// dropped, the per-reference copy of the records is made again (ctx_expand_references), then the Woop data (refit_launch_woop), the node levels
// (refit_launch_levels), the root card (ctx_refresh_root_card) and the timer marks between them; the stream is waited for and the context left as
// adypt_reset leaves it.
int refit_tail(adypt_ctx *c);
// What adypt_update_triangles_auto refuses of its params and policy, `request` being the rebuild they name: the reason as build_request.hpp gives it, or null.
const char *refit_policy_refused(const adypt_bvh_params *params, const adypt_pose_policy *policy, BuildRequest *request);
// adypt_update_triangles_auto around any refit: the reference cost, `refit` (a refit_begin .. refit_tail that has checked its own arguments), the cost
// of the refitted tree, and the rebuild `request` names where that cost is above rebuild_above times the reference.
int refit_under_policy(adypt_ctx *c, const char *who, const BuildRequest &request, double rebuild_above, adypt_pose_outcome *outcome, const std::function<int()> &refit);
// multi_each of a call that gives an outcome: *outcome is the first device's, and a device that measured or decided otherwise ends the call (ADYPT_E_HIP)
int multi_each_outcome(adypt_multi *m, const char *who, adypt_pose_outcome *outcome, const std::function<int(adypt_ctx *, adypt_pose_outcome *)> &f);

}  // namespace adypt
