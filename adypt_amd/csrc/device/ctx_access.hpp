// Internal seam between tracer.hip (owner of struct adypt_ctx) and multi.hip (RCCL gather of the tile shards): the few
// fields the collective needs, without exposing the context's layout.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

struct adypt_ctx;

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

}  // namespace adypt
