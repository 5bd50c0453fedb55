// What a translation unit beside tracer.hip is written with (denoise.hip, refit.hip, build.hip, geometry.hip, the next one): how it reports an error into the
// context, how it keeps its state in the context, how it grows a buffer and sizes a grid, how it times its stages.  Everything goes through
// ctx_access.hpp: nothing here sees the layout of adypt_ctx.  Not part of the C-ABI.
#pragma once
#include "ctx_access.hpp"
#include "resources.hpp"
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <string>

namespace adypt {

inline int ctx_fail(adypt_ctx *c, int code, const std::string &msg) { ctx_set_error(c, msg); return code; }

// A HIP call of an entry point: its failure is the call's, with the expression and HIP's text in the context's error.  Unlike context.hpp's HIP_TRY
// these give HIP's last error back before they return: a failure here (out of memory for scratch, mostly) leaves the context usable, and the next
// launch anywhere in the library is checked with hipGetLastError(), which would otherwise report this failure as that launch's.
#define CTX_TRY(c, expr)                                                                                    \
	do {                                                                                                    \
		const hipError_t e_ = (expr);                                                                       \
		if(e_ != hipSuccess) { (void)hipGetLastError(); return adypt::ctx_fail(c, e_ == hipErrorOutOfMemory ? ADYPT_E_OOM : ADYPT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } \
	} while(0)
// a step that has set the context's error itself
#define CTX_STEP(expr) do { const int r_ = (expr); if(r_ != ADYPT_OK) return r_; } while(0)

// What the unit keeps per context, parked in the context's slot `kind` (ctx_attachment), which owns it: freed by adypt_destroy, the context's device
// current.  ctx_state makes it at the first call.
template <class T> T *ctx_state_if_any(adypt_ctx *c, AttachKind kind) { return (T *)ctx_attachment(c, kind).p; }
template <class T> T *ctx_state(adypt_ctx *c, AttachKind kind)
{
	Attachment &a = ctx_attachment(c, kind);
	if(!a.p) a.reset(new T(), [](void *p) { delete (T *)p; });
	return (T *)a.p;
}

// `b` holds `count` elements, 64 bytes at the least; what it held is lost when it has to grow
template <class T> hipError_t at_least(Buffer<T> &b, size_t count)
{
	const size_t bytes = std::max<size_t>(count * sizeof(T), 64);
	return b.bytes() >= bytes ? hipSuccess : b.alloc(bytes);
}

inline unsigned grid_of(int64_t n, int per_group) { return (unsigned)((n + per_group - 1) / per_group); }

// The HIP-event times of the stages of one operation on one stream: mark k stands between stage k - 1 and stage k.  An operation invalidates the
// timer before its first mark and completes it once the stream has been waited for; in between, and after a failure, there is nothing to read.
template <int N> class StageTimer {
	Event ev_[N];
	bool complete_ = false;
public:
	// (the event is made at its first mark: the context's device is current)
	hipError_t mark(int k, hipStream_t stream)
	{
		if(!(hipEvent_t)ev_[k]) { const hipError_t e = hipEventCreate(ev_[k].out()); if(e != hipSuccess) return e; }
		return hipEventRecord(ev_[k], stream);
	}
	void invalidate() { complete_ = false; }
	void complete() { complete_ = true; }
	bool completed() const { return complete_; }
	// What adypt_get_*_timing answers (adypt_hip.h): n_parts values, stage k from mark k to mark k + 1, and with_total one more, from mark 0 to mark
	// n_parts.  Returns their number; writes them only when `capacity` holds them all.  A stage whose marks were not both recorded reads 0.
	int read(float *ms, int capacity, int n_parts, bool with_total) const
	{
		const int n = n_parts + (with_total ? 1 : 0);
		if(capacity < n) return n;
		for(int k = 0; k < n; ++k)
		{
			const bool total = k == n_parts;
			ms[k] = 0.0f;
			(void)hipEventElapsedTime(&ms[k], ev_[total ? 0 : k], ev_[total ? n_parts : k + 1]);
		}
		(void)hipGetLastError();
		return n;
	}
};

}  // namespace adypt
