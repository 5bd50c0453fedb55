// What geometry.hip needs of mesh.hip.  Not part of the C-ABI.
#pragma once

struct adypt_ctx;

namespace adypt {

// The context's triangles have been replaced (adypt_set_triangles): the index buffer and the incidence lists were the old triangles' and are given
// back; the context's device is current.  Nothing where there is no mesh binding.
void mesh_drop_binding(adypt_ctx *c);

}  // namespace adypt
