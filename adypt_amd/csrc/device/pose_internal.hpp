// What geometry.hip needs of pose.hip.  Not part of the C-ABI.
#pragma once

struct adypt_ctx;

namespace adypt {

// The context's triangles have been replaced (adypt_set_triangles): the rest pose and the binding were the old triangles' and are given back; the
// context's device is current.  Nothing where there is no binding.
void pose_drop_binding(adypt_ctx *c);

}  // namespace adypt
