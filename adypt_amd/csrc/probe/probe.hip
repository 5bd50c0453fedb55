// TEST INFRASTRUCTURE — adypt_amd/libadypt_probe.so (probe.h): one plain kernel per device helper of canon_math.hpp / shade.hpp / noise.hpp, compiled
// with the very flags of the product's device code (csrc/Makefile: DEVICE_CC), so that the helpers run here in the float mode and with the inline
// assembly they have inside the traversal and shading kernels.  Nothing of this is linked into libadypt_hip.so.
//
// At the end of the file: the denoiser's own kernels (denoise_kernels.hpp, the header denoise.hip compiles), launched as the product launches them.
//
// Every helper kernel: thread i handles element i and touches nothing but element i of its arrays (the one table — the texture — is indexed by
// sample_texture itself, whose indices are wrapped into the texture).  Every entry checks n, every HIP call and the launch.
#include "../device/shade.hpp"
#include "../device/denoise_kernels.hpp"
#include "probe.h"

#include <vector>

using namespace adypt;

namespace {

constexpr int64_t kMaxElements = 1ll << 24;
constexpr int kThreads = 256;

#define PROBE_TRY(expr) do { const hipError_t err_ = (expr); if(err_ != hipSuccess) return -(int)err_; } while(0)
#define PROBE_REQUIRE(cond) do { if(!(cond)) return -(int)hipErrorInvalidValue; } while(0)
#define PROBE_INDEX(i, n) const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; if(i >= n) return

// a device array that lives for one call
class Dev {
public:
	Dev() = default;
	Dev(const Dev &) = delete;
	Dev &operator=(const Dev &) = delete;
	~Dev() { if(p_) (void)hipFree(p_); }
	hipError_t in(const void *host, size_t bytes)
	{
		const hipError_t e = alloc(bytes);
		return e != hipSuccess || bytes == 0 ? e : hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice);
	}
	hipError_t out(size_t bytes)
	{
		const hipError_t e = alloc(bytes);
		return e != hipSuccess ? e : hipMemset(p_, 0, bytes_);
	}
	// `bytes` (a multiple of 4) of the 32-bit word `word`: an output in which what no thread wrote shows, or the slack round a table
	hipError_t filled(size_t bytes, uint32_t word)
	{
		const hipError_t e = alloc(bytes);
		return e != hipSuccess ? e : hipMemsetD32((hipDeviceptr_t)p_, (int)word, bytes_ / 4);
	}
	hipError_t put(size_t at, const void *host, size_t bytes) { return bytes == 0 ? hipSuccess : hipMemcpy((char *)p_ + at, host, bytes, hipMemcpyHostToDevice); }
	hipError_t back(void *host) const { return hipMemcpy(host, p_, bytes_, hipMemcpyDeviceToHost); }
	template <class T> T *as() const { return (T *)p_; }
private:
	hipError_t alloc(size_t bytes)
	{
		bytes_ = bytes ? bytes : 4;
		const hipError_t e = hipMalloc(&p_, bytes_);
		if(e != hipSuccess) p_ = nullptr;
		return e;
	}
	void *p_ = nullptr;
	size_t bytes_ = 0;
};

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }
inline hipError_t launched() { const hipError_t e = hipGetLastError(); return e != hipSuccess ? e : hipDeviceSynchronize(); }
template <class... P> bool none_null(P... p) { return (... && (p != nullptr)); }

// RGB8 -> the device's texel rows (upload_textures_and_materials, scene_upload.hpp): w + 1 per row, the last a copy of the first
std::vector<uint32_t> texel_rows(const uint8_t *rgb, int w, int h)
{
	const size_t row = (size_t)w + 1;
	std::vector<uint32_t> texels(row * (size_t)h);
	for(int y = 0; y < h; ++y)
	{
		uint32_t *o = texels.data() + row * (size_t)y;
		const uint8_t *in = rgb + (size_t)y * (size_t)w * 3;
		for(int x = 0; x < w; ++x) o[x] = (uint32_t)in[x * 3] | (uint32_t)in[x * 3 + 1] << 8 | (uint32_t)in[x * 3 + 2] << 16 | 0xff000000u;
		o[w] = o[0];
	}
	return texels;
}

__device__ __forceinline__ F3 ld_f3(const float *a, int64_t i) { return f3(a[3 * i], a[3 * i + 1], a[3 * i + 2]); }
__device__ __forceinline__ void st_f3(float *a, int64_t i, F3 v) { a[3 * i] = v.x; a[3 * i + 1] = v.y; a[3 * i + 2] = v.z; }

// ---- canon_math.hpp -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void p_rcp(int64_t n, const float *x, float *out) { PROBE_INDEX(i, n); out[i] = rcp_ieee(x[i]); }
__global__ __launch_bounds__(kThreads) void p_normalize(int64_t n, const float *v, float *out) { PROBE_INDEX(i, n); st_f3(out, i, normalize3(ld_f3(v, i))); }
__global__ __launch_bounds__(kThreads) void p_sincos(int64_t n, const float *x, float *s, float *c)
{
	PROBE_INDEX(i, n);
	float sv, cv;
	canon_sincos(x[i], &sv, &cv);
	s[i] = sv; c[i] = cv;
}
__global__ __launch_bounds__(kThreads) void p_pow(int64_t n, const float *x, const float *y, float *out) { PROBE_INDEX(i, n); out[i] = canon_pow(x[i], y[i]); }
__global__ __launch_bounds__(kThreads) void p_unorm8(int64_t n, const uint32_t *c, float *out) { PROBE_INDEX(i, n); out[i] = unorm8_to_float(c[i]); }
__global__ __launch_bounds__(kThreads) void p_exp_byte(int64_t n, const uint32_t *word, uint32_t *out)
{
	PROBE_INDEX(i, n);
	const uint32_t w = word[i];
	out[3 * i] = __float_as_uint(exp_byte<0>(w)); out[3 * i + 1] = __float_as_uint(exp_byte<1>(w)); out[3 * i + 2] = __float_as_uint(exp_byte<2>(w));
}
__global__ __launch_bounds__(kThreads) void p_shl_bytes(int64_t n, const uint32_t *s, const uint32_t *x, uint32_t *out)
{
	PROBE_INDEX(i, n);
	const uint32_t sv = s[i], xv = x[i];
	out[4 * i] = shl_bytes<0>(sv, xv); out[4 * i + 1] = shl_bytes<1>(sv, xv); out[4 * i + 2] = shl_bytes<2>(sv, xv); out[4 * i + 3] = shl_bytes<3>(sv, xv);
}
// or_if_le inside a divergent branch, as in the traversal loop: the lanes outside lane_mask must come out untouched, and the OR of B after the
// branch must reach every lane (EXEC restored by the helper, then by the compiler's end of the branch)
__global__ __launch_bounds__(kThreads) void p_or_if_le(int64_t n, const uint32_t *A, const float *a, const float *b, const uint32_t *bits, const uint32_t *B,
                                                       unsigned long long lane_mask, uint32_t *out)
{
	PROBE_INDEX(i, n);
	uint32_t acc = A[i];
	const float av = a[i], bv = b[i];
	const uint32_t bt = bits[i], after = B[i];
	if((lane_mask >> (threadIdx.x & 63)) & 1ull) or_if_le(acc, av, bv, bt);
	acc |= after;
	out[i] = acc;
}
__global__ __launch_bounds__(kThreads) void p_minmax(int64_t n, const float *a, const float *b, float *out)
{
	PROBE_INDEX(i, n);
	const float av = a[i], bv = b[i];
	out[4 * i] = max_num(av, bv); out[4 * i + 1] = min_num(av, bv); out[4 * i + 2] = gl_min(av, bv); out[4 * i + 3] = gl_max(av, bv);
}
__global__ __launch_bounds__(kThreads) void p_pk_fma_hi(int64_t n, const float *a, const float *b, const float *c, float *hi, float *plain)
{
	PROBE_INDEX(i, n);
	const V2 av = v2(a[2 * i], a[2 * i + 1]), bv = v2(b[2 * i], b[2 * i + 1]), cv = v2(c[2 * i], c[2 * i + 1]);
	const V2 h = pk_fma_hi(av, bv, cv), p = pk_fma(av, v2s(bv.y), cv);
	hi[2 * i] = h.x; hi[2 * i + 1] = h.y; plain[2 * i] = p.x; plain[2 * i + 1] = p.y;
}

// ---- shade.hpp ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void p_sobol2(int64_t n, const float *q, const float *s, float *out_rng, float *out_point)
{
	PROBE_INDEX(i, n);
	const float sx = s[2 * i], sy = s[2 * i + 1];
	float x, y;
	sobol2(Rng{sx, sy, q}, (int)i, &x, &y); // reads q[2 i], q[2 i + 1]
	out_rng[2 * i] = x; out_rng[2 * i + 1] = y;
	sobol2(RngPoint{sx, sy, q[2 * i], q[2 * i + 1]}, 0, &x, &y);
	out_point[2 * i] = x; out_point[2 * i + 1] = y;
}
__global__ __launch_bounds__(kThreads) void p_sample_hemisphere(int64_t n, const float *r, float e, float *out)
{
	PROBE_INDEX(i, n);
	st_f3(out, i, sample_hemisphere(RngPoint{0.0f, 0.0f, r[2 * i], r[2 * i + 1]}, 0, e));
}
__global__ __launch_bounds__(kThreads) void p_align_direction(int64_t n, const float *dir, const float *target, float *out)
{
	PROBE_INDEX(i, n);
	st_f3(out, i, align_direction(ld_f3(dir, i), ld_f3(target, i)));
}
struct ProbeMaterial { int32_t dtex; float kd[3]; int32_t etex; float ke[3]; int32_t stex; float ks[3]; int32_t illum; float shininess, dissolve, ior; };
static_assert(sizeof(ProbeMaterial) == 64, "material record of the reference");
__global__ __launch_bounds__(kThreads) void p_respond(int64_t n, const ProbeMaterial *mats, const float *normal, const float *dir_in, const float *r, int max_bounce,
                                                      float *dir_out, float *color_out, float *ret_out, int32_t *alive_out)
{
	PROBE_INDEX(i, n);
	const ProbeMaterial m = mats[i];
	SurfaceInfo si;
	si.origin = f3(0, 0, 0); si.normal = ld_f3(normal, i);
	si.diffuse = f3(m.kd[0], m.kd[1], m.kd[2]); si.specular = f3(m.ks[0], m.ks[1], m.ks[2]); si.emission = f3(m.ke[0], m.ke[1], m.ke[2]);
	si.illum0 = m.illum; si.shininess = m.shininess; si.ior = m.ior; si.bad_mat = false;
	FrameArgs f = {};
	f.max_bounce = max_bounce;
	F3 dir = ld_f3(dir_in, i), color = f3(1.0f, 1.0f, 1.0f), ret = f3(0, 0, 0);
	const bool alive = respond(f, si, RngPoint{0.0f, 0.0f, r[2 * i], r[2 * i + 1]}, 0, dir, color, ret);
	st_f3(dir_out, i, dir); st_f3(color_out, i, color); st_f3(ret_out, i, ret);
	alive_out[i] = alive ? 1 : 0;
}
__global__ __launch_bounds__(kThreads) void p_sample_texture(int64_t n, const uint32_t *texels, int w, int h, const float *s, const float *t, float *out)
{
	PROBE_INDEX(i, n);
	SceneArgs sc = {};
	sc.texels = texels;
	st_f3(out, i, sample_texture(sc, make_int4(0, w, h, 0), s[i], t[i]));
}

// ---- noise.hpp ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void p_noise(int64_t n, const float *samples, int k, int first, int n_frames, float *mean, float *m2, float *e)
{
	PROBE_INDEX(i, n);
	NoiseMoments m{0.0f, 0.0f};
	for(int j = 0; j < k; ++j)
	{
		const F3 r = ld_f3(samples, i * k + j);
		m = noise_add_sample(m, first + j, r.x, r.y, r.z);
	}
	mean[i] = m.mean; m2[i] = m.m2; e[i] = noise_of_pixel(m, n_frames);
}

} // namespace

#define PROBE_CHECK_N(n) do { PROBE_REQUIRE((n) >= 0 && (n) <= kMaxElements); if((n) == 0) return 0; } while(0)

extern "C" {

int adypt_probe_rcp(const float *x, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(x, out));
	Dev dx, dout;
	PROBE_TRY(dx.in(x, n * 4)); PROBE_TRY(dout.out(n * 4));
	p_rcp<<<grid_for(n), kThreads>>>(n, dx.as<float>(), dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_normalize(const float *v, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(v, out));
	Dev dv, dout;
	PROBE_TRY(dv.in(v, n * 12)); PROBE_TRY(dout.out(n * 12));
	p_normalize<<<grid_for(n), kThreads>>>(n, dv.as<float>(), dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_sincos(const float *x, float *s, float *c, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(x, s, c));
	Dev dx, ds, dc;
	PROBE_TRY(dx.in(x, n * 4)); PROBE_TRY(ds.out(n * 4)); PROBE_TRY(dc.out(n * 4));
	p_sincos<<<grid_for(n), kThreads>>>(n, dx.as<float>(), ds.as<float>(), dc.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(ds.back(s)); PROBE_TRY(dc.back(c));
	return 0;
}

int adypt_probe_pow(const float *x, const float *y, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(x, y, out));
	Dev dx, dy, dout;
	PROBE_TRY(dx.in(x, n * 4)); PROBE_TRY(dy.in(y, n * 4)); PROBE_TRY(dout.out(n * 4));
	p_pow<<<grid_for(n), kThreads>>>(n, dx.as<float>(), dy.as<float>(), dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_unorm8(const uint32_t *c, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(c, out));
	Dev dc, dout;
	PROBE_TRY(dc.in(c, n * 4)); PROBE_TRY(dout.out(n * 4));
	p_unorm8<<<grid_for(n), kThreads>>>(n, dc.as<uint32_t>(), dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_exp_byte(const uint32_t *word, uint32_t *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(word, out));
	Dev dw, dout;
	PROBE_TRY(dw.in(word, n * 4)); PROBE_TRY(dout.out(n * 12));
	p_exp_byte<<<grid_for(n), kThreads>>>(n, dw.as<uint32_t>(), dout.as<uint32_t>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_shl_bytes(const uint32_t *s, const uint32_t *x, uint32_t *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(s, x, out));
	Dev ds, dx, dout;
	PROBE_TRY(ds.in(s, n * 4)); PROBE_TRY(dx.in(x, n * 4)); PROBE_TRY(dout.out(n * 16));
	p_shl_bytes<<<grid_for(n), kThreads>>>(n, ds.as<uint32_t>(), dx.as<uint32_t>(), dout.as<uint32_t>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_or_if_le(const uint32_t *A, const float *a, const float *b, const uint32_t *bits, const uint32_t *B, uint64_t lane_mask, uint32_t *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(A, a, b, bits, B, out));
	Dev dA, da, db, dbits, dB, dout;
	PROBE_TRY(dA.in(A, n * 4)); PROBE_TRY(da.in(a, n * 4)); PROBE_TRY(db.in(b, n * 4)); PROBE_TRY(dbits.in(bits, n * 4)); PROBE_TRY(dB.in(B, n * 4));
	PROBE_TRY(dout.out(n * 4));
	p_or_if_le<<<grid_for(n), kThreads>>>(n, dA.as<uint32_t>(), da.as<float>(), db.as<float>(), dbits.as<uint32_t>(), dB.as<uint32_t>(),
	                                      (unsigned long long)lane_mask, dout.as<uint32_t>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_minmax(const float *a, const float *b, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(a, b, out));
	Dev da, db, dout;
	PROBE_TRY(da.in(a, n * 4)); PROBE_TRY(db.in(b, n * 4)); PROBE_TRY(dout.out(n * 16));
	p_minmax<<<grid_for(n), kThreads>>>(n, da.as<float>(), db.as<float>(), dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_pk_fma_hi(const float *a, const float *b, const float *c, float *hi, float *plain, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(a, b, c, hi, plain));
	Dev da, db, dc, dhi, dplain;
	PROBE_TRY(da.in(a, n * 8)); PROBE_TRY(db.in(b, n * 8)); PROBE_TRY(dc.in(c, n * 8)); PROBE_TRY(dhi.out(n * 8)); PROBE_TRY(dplain.out(n * 8));
	p_pk_fma_hi<<<grid_for(n), kThreads>>>(n, da.as<float>(), db.as<float>(), dc.as<float>(), dhi.as<float>(), dplain.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dhi.back(hi)); PROBE_TRY(dplain.back(plain));
	return 0;
}

int adypt_probe_sobol2(const float *q, const float *s, float *out_rng, float *out_point, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(q, s, out_rng, out_point));
	Dev dq, ds, drng, dpoint;
	PROBE_TRY(dq.in(q, n * 8)); PROBE_TRY(ds.in(s, n * 8)); PROBE_TRY(drng.out(n * 8)); PROBE_TRY(dpoint.out(n * 8));
	p_sobol2<<<grid_for(n), kThreads>>>(n, dq.as<float>(), ds.as<float>(), drng.as<float>(), dpoint.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(drng.back(out_rng)); PROBE_TRY(dpoint.back(out_point));
	return 0;
}

int adypt_probe_sample_hemisphere(const float *r, float e, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(r, out));
	Dev dr, dout;
	PROBE_TRY(dr.in(r, n * 8)); PROBE_TRY(dout.out(n * 12));
	p_sample_hemisphere<<<grid_for(n), kThreads>>>(n, dr.as<float>(), e, dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_align_direction(const float *dir, const float *target, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(dir, target, out));
	Dev dd, dt, dout;
	PROBE_TRY(dd.in(dir, n * 12)); PROBE_TRY(dt.in(target, n * 12)); PROBE_TRY(dout.out(n * 12));
	p_align_direction<<<grid_for(n), kThreads>>>(n, dd.as<float>(), dt.as<float>(), dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_respond(const void *materials, const float *normal, const float *dir_in, const float *r, int max_bounce, float *dir_out, float *color_out,
                        float *ret_out, int32_t *alive_out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(materials, normal, dir_in, r, dir_out, color_out, ret_out, alive_out));
	Dev dm, dn, dd, dr, ddir, dcol, dret, dalive;
	PROBE_TRY(dm.in(materials, n * 64)); PROBE_TRY(dn.in(normal, n * 12)); PROBE_TRY(dd.in(dir_in, n * 12)); PROBE_TRY(dr.in(r, n * 8));
	PROBE_TRY(ddir.out(n * 12)); PROBE_TRY(dcol.out(n * 12)); PROBE_TRY(dret.out(n * 12)); PROBE_TRY(dalive.out(n * 4));
	p_respond<<<grid_for(n), kThreads>>>(n, dm.as<ProbeMaterial>(), dn.as<float>(), dd.as<float>(), dr.as<float>(), max_bounce, ddir.as<float>(),
	                                     dcol.as<float>(), dret.as<float>(), dalive.as<int32_t>());
	PROBE_TRY(launched());
	PROBE_TRY(ddir.back(dir_out)); PROBE_TRY(dcol.back(color_out)); PROBE_TRY(dret.back(ret_out)); PROBE_TRY(dalive.back(alive_out));
	return 0;
}

int adypt_probe_sample_texture(const uint8_t *rgb, int w, int h, const float *s, const float *t, float *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(rgb, s, t, out));
	PROBE_REQUIRE(w > 0 && h > 0 && ((int64_t)w + 1) * (int64_t)h <= kMaxElements);
	// the layout of upload_textures_and_materials (scene_upload.hpp), which is one step of adypt_create there and not a function of its own
	const std::vector<uint32_t> texels = texel_rows(rgb, w, h);
	Dev dtex, ds, dt, dout;
	PROBE_TRY(dtex.in(texels.data(), texels.size() * 4)); PROBE_TRY(ds.in(s, n * 4)); PROBE_TRY(dt.in(t, n * 4)); PROBE_TRY(dout.out(n * 12));
	p_sample_texture<<<grid_for(n), kThreads>>>(n, dtex.as<uint32_t>(), w, h, ds.as<float>(), dt.as<float>(), dout.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_display(const float *rgba, int viewer_type, uint32_t *out, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(rgba, out));
	Dev din, dout;
	PROBE_TRY(din.in(rgba, n * 16)); PROBE_TRY(dout.out(n * 4));
	k_display<<<grid_for(n), 256>>>(din.as<float4>(), (int)n, viewer_type, dout.as<uint32_t>());
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_noise(const float *samples, int k, int first, int n_frames, float *mean, float *m2, float *e, int64_t n)
{
	PROBE_CHECK_N(n); PROBE_REQUIRE(none_null(samples, mean, m2, e));
	PROBE_REQUIRE(k >= 0 && k <= 4096 && n * (int64_t)k <= kMaxElements && first >= 0 && first <= INT32_MAX - k);
	Dev ds, dmean, dm2, de;
	PROBE_TRY(ds.in(samples, (size_t)n * (size_t)k * 12)); PROBE_TRY(dmean.out(n * 4)); PROBE_TRY(dm2.out(n * 4)); PROBE_TRY(de.out(n * 4));
	p_noise<<<grid_for(n), kThreads>>>(n, ds.as<float>(), k, first, n_frames, dmean.as<float>(), dm2.as<float>(), de.as<float>());
	PROBE_TRY(launched());
	PROBE_TRY(dmean.back(mean)); PROBE_TRY(dm2.back(m2)); PROBE_TRY(de.back(e));
	return 0;
}

} // extern "C"

// ---- denoise_kernels.hpp: the product's kernels, launched with the product's launch shapes ------------------------------------------------
namespace {

constexpr uint32_t kUnwritten = 0x7fc0deadu; // every output is filled with this quiet NaN before the launch: a pixel no thread wrote keeps it
constexpr int kMaxSide = 4096;
constexpr int64_t kSlackTris = 64;           // triangles of slack in front of and behind the gather's two tables ...
constexpr uint32_t kSlackWord = 0x4640e400u; // ... filled with 12345.0f
constexpr int64_t kMaxStray = 32;            // how far outside [0, n_known) a hit word may point (the slack is twice that)

constexpr int64_t kSlackMats = 64;           // materials of slack round the chain's material table, and elements round what it indexes by a pixel word
constexpr int kSlackTouched = 10001;         // what a chain entry answers (negated) when a word of the slack round an array it writes has changed
constexpr uint32_t kProbeSegStride = 16;     // counters of the chain's queues lie this many words apart, as the context's cursors do

bool picture_ok(int width, int height) { return width >= 1 && height >= 1 && width <= kMaxSide && height <= kMaxSide; }
int blocks_across(int width) { return (width + kBlockDim - 1) / kBlockDim; }
// a block list the kernels may be given: every block lies in the picture's grid of blocks (a kernel writes at the coordinates the list says)
bool block_list_ok(const int32_t *blocks, int n_blocks, int width, int height)
{
	if(!blocks || n_blocks < 1 || n_blocks > 4096) return false;
	const int n_grid = blocks_across(width) * blocks_across(height);
	for(int k = 0; k < n_blocks; ++k)
		if(blocks[k] < 0 || blocks[k] >= n_grid) return false;
	return true;
}

// a hit word or a pixel word a chain kernel may be given: what a failing guard would use as an index stays inside the slack — or is INT32_MAX, the one
// far word the guards are held against (as an index it lies outside every allocation of the process)
bool word_ok(int32_t word, int64_t n) { return ((int64_t)word >= -kMaxStray && (int64_t)word < n + kMaxStray) || word == INT32_MAX; }
int32_t word_of(const float *f) { int32_t w; memcpy(&w, f, 4); return w; }

// the scene of a chain entry on the device: both tables between slack, at most one texture
struct ProbeChainScene {
	Dev tris, mats, texels;
	ChainScene sc;
};
// triangles: n_tris records of kTriFloat4 float4; materials: n_mats records of kMatFloat4 float4, the fifth (texel offset, w, h, 0) of the diffuse texture
bool chain_scene_ok(const float *triangles, int64_t n_tris, const float *materials, int n_mats, const uint8_t *tex_rgb, int tex_w, int tex_h)
{
	if(!triangles || !materials || n_tris < 1 || n_tris > (1 << 20) || n_mats < 1 || n_mats > 4096) return false;
	if(tex_rgb && !(tex_w > 0 && tex_h > 0 && ((int64_t)tex_w + 1) * (int64_t)tex_h <= kMaxElements)) return false;
	for(int64_t t = 0; t < n_tris; ++t)
	{
		const int32_t matid = word_of(triangles + (size_t)t * kTriFloat4 * 4 + 18);
		if(matid < -kMaxStray || matid >= n_mats + kMaxStray) return false;
	}
	for(int m = 0; m < n_mats; ++m) // a material that names the texture describes it as the upload would
	{
		const float *mp = materials + (size_t)m * kMatFloat4 * 4;
		if(tex_rgb && word_of(mp) == 0 && !(word_of(mp + 16) == 0 && word_of(mp + 17) == tex_w && word_of(mp + 18) == tex_h)) return false;
	}
	return true;
}
hipError_t chain_scene_in(ProbeChainScene *s, const float *triangles, int64_t n_tris, const float *materials, int n_mats, const uint8_t *tex_rgb, int tex_w, int tex_h)
{
	const size_t tri = (size_t)kTriFloat4 * 16, mat = (size_t)kMatFloat4 * 16;
	hipError_t e;
	if((e = s->tris.filled((size_t)(n_tris + 2 * kSlackTris) * tri, kSlackWord)) != hipSuccess || (e = s->tris.put((size_t)kSlackTris * tri, triangles, (size_t)n_tris * tri)) != hipSuccess) return e;
	if((e = s->mats.filled((size_t)(n_mats + 2 * kSlackMats) * mat, kSlackWord)) != hipSuccess || (e = s->mats.put((size_t)kSlackMats * mat, materials, (size_t)n_mats * mat)) != hipSuccess) return e;
	if(tex_rgb)
	{
		const std::vector<uint32_t> texels = texel_rows(tex_rgb, tex_w, tex_h);
		if((e = s->texels.in(texels.data(), texels.size() * 4)) != hipSuccess) return e;
	}
	s->sc = ChainScene{s->tris.as<float4>() + kSlackTris * kTriFloat4, s->mats.as<float4>() + kSlackMats * kMatFloat4, tex_rgb ? s->texels.as<uint32_t>() : nullptr, n_tris, n_mats, tex_rgb ? 1 : 0};
	return hipSuccess;
}

// an array of n float4 elements a chain kernel indexes by a pixel word, between kSlackMats elements of slack on either side
class Slacked {
public:
	hipError_t in(const float *host, size_t n)
	{
		n_ = n;
		const hipError_t e = d_.filled((n + 2 * (size_t)kSlackMats) * 16, kSlackWord);
		return e != hipSuccess ? e : d_.put((size_t)kSlackMats * 16, host, n * 16);
	}
	float4 *get() const { return d_.as<float4>() + kSlackMats; }
	// the elements back to the host; *intact: no word of the slack has changed
	hipError_t back(float *host, bool *intact) const
	{
		std::vector<uint32_t> all((n_ + 2 * (size_t)kSlackMats) * 4);
		const hipError_t e = d_.back(all.data());
		if(e != hipSuccess) return e;
		for(size_t k = 0; k < (size_t)kSlackMats * 4; ++k)
			if(all[k] != kSlackWord || all[all.size() - 1 - k] != kSlackWord) *intact = false;
		memcpy(host, all.data() + (size_t)kSlackMats * 4, n_ * 16);
		return hipSuccess;
	}
private:
	Dev d_;
	size_t n_ = 0;
};

bool chain_queue_ok(int segments, uint32_t seg_cap) { return segments >= 1 && segments <= 64 && seg_cap >= 1 && seg_cap <= (1u << 20) && (int64_t)segments * seg_cap <= kMaxElements; }

} // namespace

extern "C" {

int adypt_probe_denoise_prepare(const float *accum, const float *moments, const float *albedo, const float *normal, const float *position, const float *hits, const int32_t *blocks,
                                const int32_t *block_spp, int n_blocks, int width, int height, float *x0, float *x1, float *x2, float *xa)
{
	PROBE_REQUIRE(none_null(accum, moments, albedo, normal, position, hits, block_spp, x0, x1, x2, xa));
	PROBE_REQUIRE(picture_ok(width, height) && block_list_ok(blocks, n_blocks, width, height));
	const int n_px = n_blocks * kBlockPixels;
	const size_t local = (size_t)n_px * 16, image = (size_t)width * height * 16;
	Dev dc, dm, da, dn, dp, dh, db, ds, o0, o1, o2, oa;
	PROBE_TRY(dc.in(accum, local)); PROBE_TRY(dm.in(moments, local / 2)); PROBE_TRY(da.in(albedo, local)); PROBE_TRY(dn.in(normal, local)); PROBE_TRY(dp.in(position, local));
	PROBE_TRY(dh.in(hits, local)); PROBE_TRY(db.in(blocks, (size_t)n_blocks * 4)); PROBE_TRY(ds.in(block_spp, (size_t)n_blocks * 4));
	PROBE_TRY(o0.filled(image, kUnwritten)); PROBE_TRY(o1.filled(image, kUnwritten)); PROBE_TRY(o2.filled(image, kUnwritten)); PROBE_TRY(oa.filled(image, kUnwritten));
	const LaunchShape shape = prepare_launch(n_px);
	hipLaunchKernelGGL(prepare_instance(false, false), shape.grid, shape.block, 0, 0, dc.as<float4>(), dm.as<float2>(), db.as<int32_t>(), ds.as<int32_t>(), n_px, blocks_across(width), width, height,
	                   da.as<float4>(), dn.as<float4>(), dp.as<float4>(), dh.as<float4>(), o0.as<float4>(), o1.as<float4>(), o2.as<float4>(), oa.as<float4>());
	PROBE_TRY(launched());
	PROBE_TRY(o0.back(x0)); PROBE_TRY(o1.back(x1)); PROBE_TRY(o2.back(x2)); PROBE_TRY(oa.back(xa));
	return 0;
}

int adypt_probe_atrous(const float *x0, const float *x1, const float *x2, const float *xa, int width, int height, int step, float sigma_l, float sigma_z, int last, float *out)
{
	PROBE_REQUIRE(none_null(x0, x1, x2, xa, out) && picture_ok(width, height) && step >= 1 && step <= (1 << kDenoiseMaxLevels));
	const size_t image = (size_t)width * height * 16;
	Dev d0, d1, d2, da, dout;
	PROBE_TRY(d0.in(x0, image)); PROBE_TRY(d1.in(x1, image)); PROBE_TRY(d2.in(x2, image)); PROBE_TRY(da.in(xa, image));
	PROBE_TRY(dout.filled(last ? image / 4 * 3 : image, kUnwritten));
	const LaunchShape shape = atrous_launch(width, height);
	// (as run_filter launches a level: the image the instance does not write is never touched)
	hipLaunchKernelGGL(atrous_instance(last != 0), shape.grid, shape.block, 0, 0, d0.as<float4>(), d1.as<float4>(), d2.as<float4>(), da.as<float4>(), last ? (float4 *)nullptr : dout.as<float4>(),
	                   last ? dout.as<float>() : (float *)nullptr, width, height, step, sigma_l, sigma_z);
	PROBE_TRY(launched());
	PROBE_TRY(dout.back(out));
	return 0;
}

int adypt_probe_rectify_window(int radius, const float *x0, const float *x1, const float *x2, const float *xa, int width, int height, const float *origin, float *r0, float *r1)
{
	PROBE_REQUIRE(none_null(x0, x1, x2, xa, origin, r0, r1) && picture_ok(width, height) && radius >= 1 && radius <= kRectifyMaxRadius);
	const size_t image = (size_t)width * height * 16;
	Dev d0, d1, d2, da, o0, o1;
	PROBE_TRY(d0.in(x0, image)); PROBE_TRY(d1.in(x1, image)); PROBE_TRY(d2.in(x2, image)); PROBE_TRY(da.in(xa, image));
	PROBE_TRY(o0.filled(image, kUnwritten)); PROBE_TRY(o1.filled(image, kUnwritten));
	RectifyOrigin o;
	for(int k = 0; k < 3; ++k) o.o[k] = origin[k];
	const LaunchShape shape = window_launch(width, height);
	hipLaunchKernelGGL(window_instance(radius), shape.grid, shape.block, 0, 0, d0.as<float4>(), d1.as<float4>(), d2.as<float4>(), da.as<float4>(), o0.as<float4>(), o1.as<float4>(), width, height, o);
	PROBE_TRY(launched());
	PROBE_TRY(o0.back(r0)); PROBE_TRY(o1.back(r1));
	return 0;
}

int adypt_probe_temporal_merge(int motion, int rectify, const float *x0, const float *x1, const float *x2, const float *xa, const float *h0, const float *h1, const float *h2, const float *ha,
                               int have, const float *origin, const float *inv_proj, const float *inv_view, float history_cap, const float *xp, const float *xn, const float *r0,
                               const float *r1, float gamma, int width, int height, float *merged, float *x2_out, float *length, float *kept)
{
	PROBE_REQUIRE(none_null(x0, x1, x2, xa, h0, h1, h2, ha, origin, inv_proj, inv_view, merged, x2_out, length) && picture_ok(width, height));
	PROBE_REQUIRE((!motion || none_null(xp, xn)) && (!rectify || none_null(r0, r1, kept)));
	const size_t image = (size_t)width * height * 16;
	Dev d0, d1, d2, da, e0, e1, e2, ea, dxp, dxn, dr0, dr1, om, ol, ok;
	PROBE_TRY(d0.in(x0, image)); PROBE_TRY(d1.in(x1, image)); PROBE_TRY(d2.in(x2, image)); PROBE_TRY(da.in(xa, image));
	PROBE_TRY(e0.in(h0, image)); PROBE_TRY(e1.in(h1, image)); PROBE_TRY(e2.in(h2, image)); PROBE_TRY(ea.in(ha, image));
	if(motion) { PROBE_TRY(dxp.in(xp, image)); PROBE_TRY(dxn.in(xn, image)); }
	if(rectify) { PROBE_TRY(dr0.in(r0, image)); PROBE_TRY(dr1.in(r1, image)); PROBE_TRY(ok.filled(image / 4, kUnwritten)); }
	PROBE_TRY(om.filled(image, kUnwritten)); PROBE_TRY(ol.filled(image / 4, kUnwritten));
	const TemporalCamera cam = temporal_camera(origin, inv_proj, inv_view);
	const LaunchShape shape = merge_launch(width, height);
	// (an instance never looks at the images of a form it is not: they are null here, as they are in a context that never made such a call)
	hipLaunchKernelGGL(merge_instance(motion != 0, rectify != 0), shape.grid, shape.block, 0, 0, d0.as<float4>(), d1.as<float4>(), d2.as<float4>(), da.as<float4>(), e0.as<float4>(), e1.as<float4>(), e2.as<float4>(),
	                   ea.as<float4>(), om.as<float4>(), ol.as<float>(), width, height, have ? 1 : 0, cam, history_cap, dxp.as<float4>(), dxn.as<float4>(), dr0.as<float4>(), dr1.as<float4>(),
	                   ok.as<float>(), gamma);
	PROBE_TRY(launched());
	PROBE_TRY(om.back(merged)); PROBE_TRY(d2.back(x2_out)); PROBE_TRY(ol.back(length));
	if(rectify) PROBE_TRY(ok.back(kept));
	return 0;
}

int adypt_probe_temporal_merge_virtual(const float *x0, const float *x1, const float *x2, const float *xa, const float *xv, const float *h0, const float *h1, const float *h2, const float *ha,
                                       int have, const float *origin, const float *inv_proj, const float *inv_view, float history_cap, int width, int height, float *merged, float *x2_out,
                                       float *length, uint64_t *counts)
{
	PROBE_REQUIRE(none_null(x0, x1, x2, xa, xv, h0, h1, h2, ha, origin, inv_proj, inv_view, merged, x2_out, length, counts) && picture_ok(width, height));
	const size_t image = (size_t)width * height * 16;
	Dev d0, d1, d2, da, dv, e0, e1, e2, ea, om, ol, oc;
	PROBE_TRY(d0.in(x0, image)); PROBE_TRY(d1.in(x1, image)); PROBE_TRY(d2.in(x2, image)); PROBE_TRY(da.in(xa, image)); PROBE_TRY(dv.in(xv, image));
	PROBE_TRY(e0.in(h0, image)); PROBE_TRY(e1.in(h1, image)); PROBE_TRY(e2.in(h2, image)); PROBE_TRY(ea.in(ha, image));
	PROBE_TRY(om.filled(image, kUnwritten)); PROBE_TRY(ol.filled(image / 4, kUnwritten)); PROBE_TRY(oc.filled(2 * kVirtualCountSlots * sizeof(unsigned long long), 0u));
	const TemporalCamera cam = temporal_camera(origin, inv_proj, inv_view);
	const LaunchShape shape = merge_launch(width, height);
	hipLaunchKernelGGL(k_temporal_merge_virtual, shape.grid, shape.block, 0, 0, d0.as<float4>(), d1.as<float4>(), d2.as<float4>(), da.as<float4>(), dv.as<float4>(), e0.as<float4>(), e1.as<float4>(),
	                   e2.as<float4>(), ea.as<float4>(), om.as<float4>(), ol.as<float>(), width, height, have ? 1 : 0, cam, history_cap, oc.as<unsigned long long>());
	PROBE_TRY(launched());
	PROBE_TRY(om.back(merged)); PROBE_TRY(d2.back(x2_out)); PROBE_TRY(ol.back(length));
	unsigned long long slots[2 * kVirtualCountSlots];
	PROBE_TRY(oc.back(slots));
	counts[0] = counts[1] = 0;
	for(int k = 0; k < kVirtualCountSlots; ++k) { counts[0] += slots[2 * k]; counts[1] += slots[2 * k + 1]; }
	return 0;
}

int adypt_probe_motion_gather(const float *hits, const float *normal, const float *position, const int32_t *blocks, int n_blocks, int width, int height, const float *snapshot,
                              int64_t n_known, const float *records, int64_t n_records, int tri_float4, float *xp, float *xn)
{
	PROBE_REQUIRE(none_null(hits, normal, position, snapshot, records, xp, xn) && picture_ok(width, height) && block_list_ok(blocks, n_blocks, width, height));
	PROBE_REQUIRE(n_known >= 0 && n_known <= n_records && n_records <= (1 << 20) && tri_float4 >= kSnapshotVecs && tri_float4 <= 64);
	const int n_px = n_blocks * kBlockPixels;
	// what a guard that fails would use as an index stays inside the slack
	for(int L = 0; L < n_px; ++L)
	{
		int32_t tri;
		memcpy(&tri, &hits[(size_t)L * 4], 4);
		PROBE_REQUIRE((int64_t)tri >= -kMaxStray && (int64_t)tri < n_known + kMaxStray);
	}
	const size_t local = (size_t)n_px * 16, image = (size_t)width * height * 16, snap_tri = (size_t)kSnapshotVecs * 16, rec_tri = (size_t)tri_float4 * 16;
	Dev dh, dn, dp, db, dsnap, drec, oxp, oxn;
	PROBE_TRY(dh.in(hits, local)); PROBE_TRY(dn.in(normal, local)); PROBE_TRY(dp.in(position, local)); PROBE_TRY(db.in(blocks, (size_t)n_blocks * 4));
	PROBE_TRY(dsnap.filled((size_t)(n_known + 2 * kSlackTris) * snap_tri, kSlackWord)); PROBE_TRY(dsnap.put((size_t)kSlackTris * snap_tri, snapshot, (size_t)n_known * snap_tri));
	PROBE_TRY(drec.filled((size_t)(n_records + 2 * kSlackTris) * rec_tri, kSlackWord)); PROBE_TRY(drec.put((size_t)kSlackTris * rec_tri, records, (size_t)n_records * rec_tri));
	PROBE_TRY(oxp.filled(image, kUnwritten)); PROBE_TRY(oxn.filled(image, kUnwritten));
	const LaunchShape shape = gather_launch(n_px);
	hipLaunchKernelGGL(k_motion_gather, shape.grid, shape.block, 0, 0, dh.as<float4>(), dn.as<float4>(), dp.as<float4>(), db.as<int32_t>(), n_px, blocks_across(width), width, height,
	                   dsnap.as<float4>() + kSlackTris * kSnapshotVecs, n_known, drec.as<float4>() + kSlackTris * tri_float4, tri_float4, oxp.as<float4>(), oxn.as<float4>());
	PROBE_TRY(launched());
	PROBE_TRY(oxp.back(xp)); PROBE_TRY(oxn.back(xn));
	return 0;
}

int adypt_probe_motion_snapshot(const float *records, int tri_float4, int64_t n_tris, float *snapshot)
{
	PROBE_REQUIRE(none_null(records, snapshot) && n_tris >= 1 && n_tris <= (1 << 20) && tri_float4 >= kSnapshotVecs && tri_float4 <= 64);
	Dev drec, dsnap;
	PROBE_TRY(drec.in(records, (size_t)n_tris * tri_float4 * 16)); PROBE_TRY(dsnap.filled((size_t)n_tris * kSnapshotVecs * 16, kUnwritten));
	const LaunchShape shape = snapshot_launch(n_tris);
	hipLaunchKernelGGL(k_motion_snapshot, shape.grid, shape.block, 0, 0, drec.as<float4>(), tri_float4, n_tris, dsnap.as<float4>());
	PROBE_TRY(launched());
	PROBE_TRY(dsnap.back(snapshot));
	return 0;
}

int adypt_probe_denoise_prepare_instance(int instance, const float *accum, const float *moments, const float *albedo, const float *normal, const float *position, const float *hits,
                                         const int32_t *blocks, const int32_t *block_spp, int n_blocks, int width, int height, float *x0, float *x1, float *x2, float *xa,
                                         const float *g_virtual, float *xv)
{
	PROBE_REQUIRE(instance >= ADYPT_PROBE_PREPARE_CLASS && instance <= ADYPT_PROBE_PREPARE_VIRTUAL);
	PROBE_REQUIRE(none_null(accum, moments, albedo, normal, position, hits, block_spp, x0, x1, x2, xa));
	PROBE_REQUIRE(instance != ADYPT_PROBE_PREPARE_VIRTUAL || none_null(g_virtual, xv));
	PROBE_REQUIRE(picture_ok(width, height) && block_list_ok(blocks, n_blocks, width, height));
	const int n_px = n_blocks * kBlockPixels;
	const size_t local = (size_t)n_px * 16, image = (size_t)width * height * 16;
	Dev dc, dm, da, dn, dp, dh, db, ds, dv, o0, o1, o2, oa, ov;
	PROBE_TRY(dc.in(accum, local)); PROBE_TRY(dm.in(moments, local / 2)); PROBE_TRY(da.in(albedo, local)); PROBE_TRY(dn.in(normal, local)); PROBE_TRY(dp.in(position, local));
	PROBE_TRY(dh.in(hits, local)); PROBE_TRY(db.in(blocks, (size_t)n_blocks * 4)); PROBE_TRY(ds.in(block_spp, (size_t)n_blocks * 4));
	PROBE_TRY(o0.filled(image, kUnwritten)); PROBE_TRY(o1.filled(image, kUnwritten)); PROBE_TRY(o2.filled(image, kUnwritten)); PROBE_TRY(oa.filled(image, kUnwritten));
	const LaunchShape shape = prepare_launch(n_px);
	if(instance == ADYPT_PROBE_PREPARE_VIRTUAL)
	{
		PROBE_TRY(dv.in(g_virtual, local)); PROBE_TRY(ov.filled(image, kUnwritten));
		hipLaunchKernelGGL(k_denoise_prepare_virtual, shape.grid, shape.block, 0, 0, dc.as<float4>(), dm.as<float2>(), db.as<int32_t>(), ds.as<int32_t>(), n_px, blocks_across(width), width, height,
		                   da.as<float4>(), dn.as<float4>(), dp.as<float4>(), dh.as<float4>(), o0.as<float4>(), o1.as<float4>(), o2.as<float4>(), oa.as<float4>(), dv.as<float4>(), ov.as<float4>());
	}
	else
		hipLaunchKernelGGL(prepare_instance(instance == ADYPT_PROBE_PREPARE_MOMENTS, instance == ADYPT_PROBE_PREPARE_CLASS), shape.grid, shape.block, 0, 0, dc.as<float4>(), dm.as<float2>(),
		                   db.as<int32_t>(), ds.as<int32_t>(), n_px, blocks_across(width), width, height, da.as<float4>(), dn.as<float4>(), dp.as<float4>(), dh.as<float4>(), o0.as<float4>(),
		                   o1.as<float4>(), o2.as<float4>(), oa.as<float4>());
	PROBE_TRY(launched());
	PROBE_TRY(o0.back(x0)); PROBE_TRY(o1.back(x1)); PROBE_TRY(o2.back(x2)); PROBE_TRY(oa.back(xa));
	if(instance == ADYPT_PROBE_PREPARE_VIRTUAL) PROBE_TRY(ov.back(xv));
	return 0;
}

int adypt_probe_temporal_merge_moments(int motion, const float *x0, const float *x1, const float *x2, const float *xa, const float *h0, const float *h1, const float *h2, const float *ha,
                                       int have, const float *origin, const float *inv_proj, const float *inv_view, float history_cap, const float *xp, const float *xn, int width,
                                       int height, float *merged, float *x2_out, float *length)
{
	PROBE_REQUIRE(none_null(x0, x1, x2, xa, h0, h1, h2, ha, origin, inv_proj, inv_view, merged, x2_out, length) && picture_ok(width, height));
	PROBE_REQUIRE(!motion || none_null(xp, xn));
	const size_t image = (size_t)width * height * 16;
	Dev d0, d1, d2, da, e0, e1, e2, ea, dxp, dxn, om, ol;
	PROBE_TRY(d0.in(x0, image)); PROBE_TRY(d1.in(x1, image)); PROBE_TRY(d2.in(x2, image)); PROBE_TRY(da.in(xa, image));
	PROBE_TRY(e0.in(h0, image)); PROBE_TRY(e1.in(h1, image)); PROBE_TRY(e2.in(h2, image)); PROBE_TRY(ea.in(ha, image));
	if(motion) { PROBE_TRY(dxp.in(xp, image)); PROBE_TRY(dxn.in(xn, image)); }
	PROBE_TRY(om.filled(image, kUnwritten)); PROBE_TRY(ol.filled(image / 4, kUnwritten));
	const TemporalCamera cam = temporal_camera(origin, inv_proj, inv_view);
	const LaunchShape shape = merge_launch(width, height);
	// (the instance without motion never looks at XP, XN: they are null here, as in a context that never followed motion)
	hipLaunchKernelGGL(merge_moments_instance(motion != 0), shape.grid, shape.block, 0, 0, d0.as<float4>(), d1.as<float4>(), d2.as<float4>(), da.as<float4>(),
	                   e0.as<float4>(), e1.as<float4>(), e2.as<float4>(), ea.as<float4>(), om.as<float4>(), ol.as<float>(), width, height, have ? 1 : 0, cam, history_cap, dxp.as<float4>(),
	                   dxn.as<float4>());
	PROBE_TRY(launched());
	PROBE_TRY(om.back(merged)); PROBE_TRY(d2.back(x2_out)); PROBE_TRY(ol.back(length));
	return 0;
}

int adypt_probe_moments_variance(const float *merged, const float *x1, const float *x2, const float *xa, int width, int height, const float *origin, float *out, float *variance,
                                 uint64_t *spatial_count)
{
	PROBE_REQUIRE(none_null(merged, x1, x2, xa, origin, out, variance, spatial_count) && picture_ok(width, height));
	const size_t image = (size_t)width * height * 16;
	Dev dm, d1, d2, da, oo, ov, oc;
	PROBE_TRY(dm.in(merged, image)); PROBE_TRY(d1.in(x1, image)); PROBE_TRY(d2.in(x2, image)); PROBE_TRY(da.in(xa, image));
	PROBE_TRY(oo.filled(image, kUnwritten)); PROBE_TRY(ov.filled(image / 4, kUnwritten)); PROBE_TRY(oc.filled(kMomentsCountSlots * sizeof(unsigned long long), 0u));
	RectifyOrigin o;
	for(int k = 0; k < 3; ++k) o.o[k] = origin[k];
	const LaunchShape shape = variance_launch(width, height);
	hipLaunchKernelGGL(k_moments_variance, shape.grid, shape.block, 0, 0, dm.as<float4>(), d1.as<float4>(), d2.as<float4>(), da.as<float4>(), oo.as<float4>(), ov.as<float>(),
	                   oc.as<unsigned long long>(), width, height, o);
	PROBE_TRY(launched());
	PROBE_TRY(oo.back(out)); PROBE_TRY(ov.back(variance));
	unsigned long long slots[kMomentsCountSlots];
	PROBE_TRY(oc.back(slots));
	*spatial_count = 0;
	for(int k = 0; k < kMomentsCountSlots; ++k) *spatial_count += slots[k];
	return 0;
}

int adypt_probe_chain_start(int unfold, const float *triangles, int64_t n_tris, const float *materials, int n_mats, const uint8_t *tex_rgb, int tex_w, int tex_h, float *albedo,
                            float *normal, float *position, float *hits, const int32_t *blocks, int n_blocks, int width, int height, const float *origin, float tmin, int bounces,
                            int segments, uint32_t seg_cap, float *state, float *queue_o, float *queue_d, uint32_t *queue_count, uint64_t *counts)
{
	PROBE_REQUIRE(none_null(albedo, normal, position, hits, origin, state, queue_o, queue_d, queue_count, counts));
	PROBE_REQUIRE(picture_ok(width, height) && block_list_ok(blocks, n_blocks, width, height) && n_blocks <= 64 && chain_bounces_valid(bounces) && chain_queue_ok(segments, seg_cap));
	PROBE_REQUIRE(chain_scene_ok(triangles, n_tris, materials, n_mats, tex_rgb, tex_w, tex_h));
	const int n_px = n_blocks * kBlockPixels;
	for(int L = 0; L < n_px; ++L) PROBE_REQUIRE(word_ok(word_of(hits + (size_t)L * 4), n_tris));
	const size_t local = (size_t)n_px * 16, queue = (size_t)segments * seg_cap * 16, cursors = (size_t)segments * kProbeSegStride * 4;
	ProbeChainScene scene;
	PROBE_TRY(chain_scene_in(&scene, triangles, n_tris, materials, n_mats, tex_rgb, tex_w, tex_h));
	Dev da, dn, dp, dh, db, ds, qo, qd, qc, dc;
	PROBE_TRY(da.in(albedo, local)); PROBE_TRY(dn.in(normal, local)); PROBE_TRY(dp.in(position, local)); PROBE_TRY(dh.in(hits, local)); PROBE_TRY(db.in(blocks, (size_t)n_blocks * 4));
	PROBE_TRY(ds.filled(2 * local, kUnwritten)); PROBE_TRY(qo.filled(queue, kUnwritten)); PROBE_TRY(qd.filled(queue, kUnwritten)); PROBE_TRY(qc.filled(cursors, 0u));
	PROBE_TRY(dc.filled(sizeof(ChainCounts), 0u));
	const ChainGuides g{da.as<float4>(), dn.as<float4>(), dp.as<float4>(), dh.as<float4>()};
	const ChainQueue out{qo.as<float4>(), qd.as<float4>(), qc.as<uint32_t>(), seg_cap, kProbeSegStride, segments};
	const ChainOrigin o{{origin[0], origin[1], origin[2]}, tmin};
	const LaunchShape shape = chain_start_launch(n_px);
	hipLaunchKernelGGL(chain_start_instance(unfold != 0), shape.grid, shape.block, 0, 0, scene.sc, g, db.as<int32_t>(), n_px, blocks_across(width), width, height, o, bounces,
	                   ds.as<float4>(), out, dc.as<ChainCounts>());
	PROBE_TRY(launched());
	PROBE_TRY(da.back(albedo)); PROBE_TRY(dn.back(normal)); PROBE_TRY(dp.back(position)); PROBE_TRY(dh.back(hits));
	PROBE_TRY(ds.back(state)); PROBE_TRY(qo.back(queue_o)); PROBE_TRY(qd.back(queue_d)); PROBE_TRY(qc.back(queue_count));
	ChainCounts c;
	PROBE_TRY(dc.back(&c));
	counts[0] = c.rays; counts[1] = c.followed; counts[2] = c.escaped; counts[3] = c.truncated;
	return 0;
}

int adypt_probe_chain_step(int unfold, const float *triangles, int64_t n_tris, const float *materials, int n_mats, const uint8_t *tex_rgb, int tex_w, int tex_h, float *albedo,
                           float *normal, float *position, float *hits, int n_px, int segments, uint32_t seg_cap, const float *in_o, const float *in_d, const float *in_hit,
                           const uint32_t *in_count, int bounces, float tmin, float *state, float *out_o, float *out_d, uint32_t *out_count, uint64_t *counts, float *virt,
                           const float *origin)
{
	PROBE_REQUIRE(none_null(albedo, normal, position, hits, in_o, in_d, in_hit, in_count, state, out_o, out_d, out_count, counts) && (!unfold || none_null(virt, origin)));
	PROBE_REQUIRE(n_px >= 1 && n_px <= (1 << 22) && chain_bounces_valid(bounces) && chain_queue_ok(segments, seg_cap));
	PROBE_REQUIRE(chain_scene_ok(triangles, n_tris, materials, n_mats, tex_rgb, tex_w, tex_h));
	const size_t slots = (size_t)segments * seg_cap;
	for(size_t k = 0; k < slots; ++k) PROBE_REQUIRE(word_ok(word_of(in_d + k * 4 + 3), n_px) && word_ok(word_of(in_hit + k * 4), n_tris));
	const size_t queue = slots * 16, cursors = (size_t)segments * kProbeSegStride * 4;
	ProbeChainScene scene;
	PROBE_TRY(chain_scene_in(&scene, triangles, n_tris, materials, n_mats, tex_rgb, tex_w, tex_h));
	Slacked da, dn, dp, dh, ds, dv;
	Dev io, id, ih, ic, qo, qd, qc, dc;
	PROBE_TRY(da.in(albedo, n_px)); PROBE_TRY(dn.in(normal, n_px)); PROBE_TRY(dp.in(position, n_px)); PROBE_TRY(dh.in(hits, n_px)); PROBE_TRY(ds.in(state, 2 * (size_t)n_px));
	if(unfold) PROBE_TRY(dv.in(virt, n_px));
	PROBE_TRY(io.in(in_o, queue)); PROBE_TRY(id.in(in_d, queue)); PROBE_TRY(ih.in(in_hit, queue)); PROBE_TRY(ic.in(in_count, cursors));
	PROBE_TRY(qo.filled(queue, kUnwritten)); PROBE_TRY(qd.filled(queue, kUnwritten)); PROBE_TRY(qc.filled(cursors, 0u)); PROBE_TRY(dc.filled(sizeof(ChainCounts), 0u));
	const ChainGuides g{da.get(), dn.get(), dp.get(), dh.get()};
	const ChainQueue in{io.as<float4>(), id.as<float4>(), ic.as<uint32_t>(), seg_cap, kProbeSegStride, segments};
	const ChainQueue out{qo.as<float4>(), qd.as<float4>(), qc.as<uint32_t>(), seg_cap, kProbeSegStride, segments};
	ChainUnfold u{unfold ? dv.get() : nullptr, {0.0f, 0.0f, 0.0f}};
	if(unfold) for(int k = 0; k < 3; ++k) u.o[k] = origin[k];
	const LaunchShape shape = chain_step_launch(segments, seg_cap); // (seg_cap: the most rays a segment can hold)
	hipLaunchKernelGGL(chain_step_instance(unfold != 0), shape.grid, shape.block, 0, 0, scene.sc, g, in, ih.as<float4>(), n_px, bounces, tmin, ds.get(), out,
	                   dc.as<ChainCounts>(), u);
	PROBE_TRY(launched());
	bool intact = true;
	PROBE_TRY(da.back(albedo, &intact)); PROBE_TRY(dn.back(normal, &intact)); PROBE_TRY(dp.back(position, &intact)); PROBE_TRY(dh.back(hits, &intact)); PROBE_TRY(ds.back(state, &intact));
	if(unfold) PROBE_TRY(dv.back(virt, &intact));
	PROBE_TRY(qo.back(out_o)); PROBE_TRY(qd.back(out_d)); PROBE_TRY(qc.back(out_count));
	ChainCounts c;
	PROBE_TRY(dc.back(&c));
	counts[0] = c.rays; counts[1] = c.followed; counts[2] = c.escaped; counts[3] = c.truncated;
	return intact ? 0 : -kSlackTouched;
}

} // extern "C"
