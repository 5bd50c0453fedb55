// What geometry.hip needs of denoise.hip.  Not part of the C-ABI.
#pragma once

struct adypt_ctx;

namespace adypt {

// The context's triangles have been replaced (adypt_set_triangles): the snapshot a committing adypt_denoise_temporal_motion left was of the old
// triangles — an index now means another triangle — and is given back; the context's device is current.  The history itself stays, as it does for
// adypt_denoise_temporal.  Nothing where there is no snapshot.
void denoise_triangles_replaced(adypt_ctx *c);

}  // namespace adypt
