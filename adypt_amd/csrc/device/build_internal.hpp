// What geometry.hip needs of build.hip: the build of a tree from triangle records that are not the context's yet.  Not part of the C-ABI.
#pragma once
#include "ctx_access.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

namespace adypt {

// The rebuild of adypt_rebuild_bvh (radius 0), adypt_rebuild_bvh_ploc and adypt_rebuild_bvh_ploc_split, whose checks of the arguments the caller has
// made, of the geometry->n_tris records at `triangles` (device memory, complete on the context's stream) instead of the context's: the context takes the
// tree and `geometry` together (ctx_replace_geometry).  After a failure the context has changed in nothing but its error and the builder's scratch.
int build_for_triangles(adypt_ctx *c, const adypt_bvh_params &cfg, int radius, double split_budget, const char *who, const float4 *triangles, NewGeometry *geometry,
                        adypt_rebuild_info *out);

}  // namespace adypt
