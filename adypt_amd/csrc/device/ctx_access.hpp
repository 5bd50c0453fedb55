// Internal seam between tracer.hip (owner of struct adypt_ctx) and multi.hip (RCCL gather of the tile shards): the few
// fields the collective needs, without exposing the context's layout.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

struct adypt_ctx;
struct adypt_multi;

namespace adypt {

struct BlockState; // active_blocks.hpp

struct CtxInfo {
	int device;
	hipStream_t stream;            // the context's own (non-blocking) stream: collectives are enqueued behind the rendering
	int rank, nranks, width, height;
	int n_local_px;                // owned blocks x 1024
	float4 *accum;                 // compact block-major running mean (image 0) of the owned blocks
};

CtxInfo ctx_info(adypt_ctx *c);
void ctx_set_error(adypt_ctx *c, const std::string &msg);
// where multi.hip parks its per-context communicator (freed by adypt_destroy through *free_fn)
void **ctx_comm_slot(adypt_ctx *c, void (***free_fn)(void *));
// adaptive sampling, per context (adypt_trace_adaptive and adypt_multi_trace_adaptive are one loop over these: active_blocks.hpp).
// ready: ADYPT_OK, or ADYPT_E_STATE with the context's error set (statistics off, look-ahead); read: APPENDS the owned blocks, ascending, each at its
// own sample count; freeze: the owned blocks among the image blocks given stop at `spp` frames.
int ctx_adaptive_ready(adypt_ctx *c, const char *fn);
int ctx_read_blocks(adypt_ctx *c, std::vector<BlockState> *blocks);
int ctx_freeze_blocks(adypt_ctx *c, const int32_t *blocks, size_t n, int spp);

// The denoiser (denoise.hip), per context.  slot: where its images are parked (freed by adypt_destroy through *free_fn).  ready: ADYPT_OK, or
// ADYPT_E_STATE with the reason in the context's error (statistics off, a viewer's image, a block below 2 spp).  inputs: the block-major local images
// the filter reads and every owned block's sample count.  capture_guides: see tracer.hip.
struct DenoiseInputs {
	const float4 *accum;               // running mean per local pixel
	const float2 *moments;             // luminance (mean, m2) per local pixel
	const int32_t *blocks;             // device: image block index of every owned block
	int n_blocks;
	std::vector<int32_t> block_index;  // host copy of `blocks`
	std::vector<int32_t> block_spp;    // samples in every owned block
};
void **ctx_denoise_slot(adypt_ctx *c, void (***free_fn)(void *));
int ctx_denoise_ready(adypt_ctx *c, const char *fn);
DenoiseInputs ctx_denoise_inputs(adypt_ctx *c);
int ctx_capture_guides(adypt_ctx *c, const char *fn, float4 *albedo, float4 *normal, float4 *position, float4 *hits);
// multi.hip: the message adypt_multi_last_error answers
void multi_set_error(adypt_multi *m, const std::string &msg);

}  // namespace adypt
