// What refit.hip and geometry.hip need of build.hip: the build a request (build_request.hpp) names, of the context's own triangles or of records that
// are not the context's yet.  The caller has made the request's checks.  Not part of the C-ABI.
#pragma once
#include "build_request.hpp"
#include "ctx_access.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

namespace adypt {

// the public rebuild a request has the shape of: the name a rebuild on behalf of a pose policy fails under
inline const char *rebuild_entry(const BuildRequest &q) { return q.method == kBuildLinear ? "adypt_rebuild_bvh" : q.split_budget == 0.0 ? "adypt_rebuild_bvh_ploc" : "adypt_rebuild_bvh_ploc_split"; }
// The rebuild of adypt_rebuild_bvh, _ploc and _ploc_split: a new tree of the context's triangles as they are now, on the context's device.  After a
// failure the context has changed in nothing but its error and the builder's scratch.
int rebuild_own_triangles(adypt_ctx *c, const BuildRequest &request, const char *who, adypt_rebuild_info *out);
// The same build of the geometry->n_tris records at `triangles` (device memory, complete on the context's stream) instead of the context's: the context
// takes the tree and `geometry` together (ctx_replace_geometry).
int build_for_triangles(adypt_ctx *c, const BuildRequest &request, const char *who, const float4 *triangles, NewGeometry *geometry, adypt_rebuild_info *out);

}  // namespace adypt
