// What build.hip needs of refit.hip: the two kernels that turn a topology plus triangles into Woop data and node records, and the hand-over of a new
// tree's level lists and exact boxes to the context's refit state.  Not part of the C-ABI.
#pragma once
#include "ctx_access.hpp"
#include "resources.hpp"

namespace adypt {

// k_refit_woop: one thread per reference
hipError_t refit_launch_woop(hipStream_t stream, const float4 *triangles, int tri_float4, const int32_t *tri_indices, int64_t n_refs, float4 *woop);
// k_refit_nodes for the nodes level[0 .. n_level) of one level; the levels below it have been launched on the same stream before
hipError_t refit_launch_nodes(hipStream_t stream, uint4 *nodes, float4 *boxes, const int32_t *level, int64_t n_level, const int32_t *tri_indices, const float4 *triangles, int tri_float4);
// The context's tree has been replaced: its refit plan is now level_begin (levels + 1 entries) over `order` (the nodes level by level, any order inside
// a level), its exact boxes are `boxes` (2 float4 per node).  Both buffers are taken.  A later adypt_update_triangles refits the new topology.
int refit_adopt_tree(adypt_ctx *c, const std::vector<int64_t> &level_begin, Buffer<int32_t> &&order, Buffer<float4> &&boxes);

}  // namespace adypt
