// TEST INFRASTRUCTURE — adypt_amd/libadypt_probe.so (probe.h): one plain kernel per device helper of canon_math.hpp / shade.hpp / noise.hpp, compiled
// with the very flags of the product's device code (csrc/Makefile: DEVICE_CC), so that the helpers run here in the float mode and with the inline
// assembly they have inside the traversal and shading kernels.  Nothing of this is linked into libadypt_hip.so.
//
// Every kernel: thread i handles element i and touches nothing but element i of its arrays (the one table — the texture — is indexed by
// sample_texture itself, whose indices are wrapped into the texture).  Every entry checks n, every HIP call and the launch.
#include "../device/shade.hpp"
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
	const size_t row = (size_t)w + 1;
	std::vector<uint32_t> texels(row * (size_t)h);
	for(int y = 0; y < h; ++y)
	{
		uint32_t *o = texels.data() + row * (size_t)y;
		const uint8_t *in = rgb + (size_t)y * (size_t)w * 3;
		for(int x = 0; x < w; ++x) o[x] = (uint32_t)in[x * 3] | (uint32_t)in[x * 3 + 1] << 8 | (uint32_t)in[x * 3 + 2] << 16 | 0xff000000u;
		o[w] = o[0];
	}
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
