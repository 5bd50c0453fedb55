// Move-only owners of what the HIP runtime hands out: device and pinned host memory, events, streams.  The ONLY place of csrc/device
// that gives any of them back.  An owner converts to the raw pointer / handle, so it is passed to the runtime and to kernels as such.
// The device an owner was filled on must be current when it releases (adypt_destroy and free_comm set it before they delete).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

namespace adypt {

// `bytes` of device memory (or of pinned host memory) seen as an array of T
template <class T, bool kPinned = false> class Buffer {
	T *p_ = nullptr;
	size_t bytes_ = 0;
public:
	Buffer() = default;
	Buffer(Buffer &&o) noexcept { *this = std::move(o); }
	Buffer &operator=(Buffer &&o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; } // (what was held goes with `o`)
	~Buffer() { release(); }
	void release() { if(p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; bytes_ = 0; }
	// gives back what is held FIRST (the peak is never old + new), then allocates; empty after a failure.  `flags`: of hipHostMalloc
	hipError_t alloc(size_t bytes, unsigned flags = 0)
	{
		release();
		const hipError_t e = kPinned ? hipHostMalloc((void **)&p_, bytes, flags) : hipMalloc((void **)&p_, bytes);
		if(e != hipSuccess) p_ = nullptr; else bytes_ = bytes;
		return e;
	}
	size_t bytes() const { return bytes_; }
	operator T *() const { return p_; }
	T *get() const { return p_; } // (where the array is to be seen as another type: a cast needs the pointer itself)
	T *operator->() const { return p_; }
};
template <class T> using PinnedBuffer = Buffer<T, true>;

// an event or a stream: created into out(), destroyed with the owner
template <class H, hipError_t (*Destroy)(H)> class Handle {
	H h_ = nullptr;
public:
	Handle() = default;
	Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
	Handle &operator=(Handle &&o) noexcept { std::swap(h_, o.h_); return *this; }
	~Handle() { if(h_) (void)Destroy(h_); }
	H *out() { return &h_; } // for hipEventCreate* / hipStreamCreate* on an EMPTY owner
	operator H() const { return h_; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

}  // namespace adypt
