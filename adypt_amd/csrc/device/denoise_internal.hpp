// What geometry.hip and history_plan.hip need of denoise.hip.  Not part of the C-ABI.
#pragma once
#include "temporal.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

struct adypt_ctx;
struct adypt_multi;

namespace adypt {

// The context's triangles have been replaced (adypt_set_triangles): the snapshot a committing adypt_denoise_temporal_motion left was of the old
// triangles — an index now means another triangle — and is given back; the context's device is current.  The history itself stays, as it does for
// adypt_denoise_temporal.  Nothing where there is no snapshot.
void denoise_triangles_replaced(adypt_ctx *c);

// What the plan by history (history_plan.hip) reads: the block-major guides of a set of blocks as ctx_capture_guides fills them — the denoiser's own
// scratch, which the next denoise call captures again — and the history a temporal call of the kind {moments, 0} would find: its four row-major
// images, its camera and, for the motion form, its snapshot.  have == 0: there is none (no denoiser yet, no history yet, one of another kind); the
// pointers may then be null.  Nothing of the history is written.
struct PlanInputs {
	const float4 *albedo, *normal, *position, *hits; // one float4 per local pixel
	const int32_t *blocks;                           // device: the image block index of every block of the set
	int n_blocks;
	std::vector<int32_t> block_index;                // host copy of `blocks`
	const float4 *h0, *h1, *h2, *ha;
	TemporalCamera camera;
	int have;
	const float4 *snapshot;
	int64_t known_tris;                              // the triangles of the snapshot the motion form may trust; 0: none
};
// the context's own blocks: the guides are captured on its stream behind whatever it holds, nothing is waited for (the context's device is current)
int denoise_plan_inputs(adypt_ctx *c, const char *fn, bool moments, PlanInputs *out);
// every block of the image, on the first device: every device captures its own, the host brings them back to back (rank order) and uploads them as
// adypt_multi_denoise does; the first device is current and its stream drained when it returns
int denoise_plan_inputs_multi(adypt_multi *m, const char *fn, bool moments, PlanInputs *out);

}  // namespace adypt
