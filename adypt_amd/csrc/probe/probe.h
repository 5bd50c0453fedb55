/* TEST INFRASTRUCTURE — C-ABI of adypt_amd/libadypt_probe.so: the device helpers of csrc/device (canon_math.hpp, shade.hpp, noise.hpp), one
 * entry per helper, so that tests/test_gpu_device_probes.py can hold each of them against the oracle's piece (oracle/oracle.cpp: orc_*) and
 * against truths that need neither side.  The product never links, loads or calls this library.
 *
 * Every entry: host pointers in and out, n elements (0 <= n <= 2^24).  It allocates, copies in, launches ONE grid of 256-thread workgroups
 * (element i = thread i), synchronises, copies out and frees; nothing is kept between calls, nothing is read from the environment.
 * Returns 0, or the negative hipError_t of the first call that failed (-1 = hipErrorInvalidValue for a bad n, size or null pointer).
 * Arrays of vectors are packed: 3 floats per element for directions and colours, 2 for Sobol points and V2 pairs. */
#ifndef ADYPT_PROBE_H
#define ADYPT_PROBE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int adypt_probe_rcp(const float *x, float *out, int64_t n);                              /* rcp_ieee */
int adypt_probe_normalize(const float *v, float *out, int64_t n);                        /* normalize3 */
int adypt_probe_sincos(const float *x, float *s, float *c, int64_t n);                   /* canon_sincos */
int adypt_probe_pow(const float *x, const float *y, float *out, int64_t n);              /* canon_pow */
int adypt_probe_unorm8(const uint32_t *c, float *out, int64_t n);                        /* unorm8_to_float (the whole word goes in) */
int adypt_probe_exp_byte(const uint32_t *word, uint32_t *out, int64_t n);                /* out[3 i + J] = bits of exp_byte<J>(word) */
int adypt_probe_shl_bytes(const uint32_t *s, const uint32_t *x, uint32_t *out, int64_t n); /* out[4 i + J] = shl_bytes<J>(s, x) */
/* acc = A; if(lane_mask bit of the thread's lane) or_if_le(acc, a, b, bits); acc |= B; out = acc.  Lane = thread index & 63. */
int adypt_probe_or_if_le(const uint32_t *A, const float *a, const float *b, const uint32_t *bits, const uint32_t *B, uint64_t lane_mask,
                         uint32_t *out, int64_t n);
int adypt_probe_minmax(const float *a, const float *b, float *out, int64_t n);           /* out[4 i ..] = max_num, min_num, gl_min, gl_max */
/* hi = pk_fma_hi(a, b, c), plain = pk_fma(a, v2s(b.y), c); V2 = 2 floats */
int adypt_probe_pk_fma_hi(const float *a, const float *b, const float *c, float *hi, float *plain, int64_t n);
/* Sobol(i) of point q[i] with shift s[i]: through Rng (the point read from the device array q at index i) and through RngPoint */
int adypt_probe_sobol2(const float *q, const float *s, float *out_rng, float *out_point, int64_t n);
int adypt_probe_sample_hemisphere(const float *r, float e, float *out, int64_t n);       /* sample_hemisphere(RngPoint{0, 0, r.x, r.y}, 0, e) */
int adypt_probe_align_direction(const float *dir, const float *target, float *out, int64_t n);
/* respond<RngPoint> at bounce 0 with colour 1 and radiance 0 going in.  materials: the 64-byte record of the reference (Kd / Ks / Ke / illum /
 * Ns / Ni are used).  Out: the new direction, the throughput, the radiance `ret` (3 floats each) and alive (1 / 0). */
int adypt_probe_respond(const void *materials, const float *normal, const float *dir_in, const float *r, int max_bounce, float *dir_out,
                        float *color_out, float *ret_out, int32_t *alive_out, int64_t n);
/* sample_texture over ONE w x h RGB8 texture (rgb: h rows of w texels, 3 bytes each), laid out for the device as scene_upload.hpp does:
 * RGBA8 words, every row w + 1 long, its last texel a copy of its first.  (w + 1) * h <= 2^24. */
int adypt_probe_sample_texture(const uint8_t *rgb, int w, int h, const float *s, const float *t, float *out, int64_t n);
int adypt_probe_display(const float *rgba, int viewer_type, uint32_t *out, int64_t n);   /* the k_display kernel: one RGBA8 word per element */
/* per element: noise_add_sample over its k samples (samples[(i * k + j) * 3 ..], frame index first + j) from moments (0, 0), then
 * noise_of_pixel(moments, n_frames).  0 <= k <= 4096. */
int adypt_probe_noise(const float *samples, int k, int first, int n_frames, float *mean, float *m2, float *e, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
