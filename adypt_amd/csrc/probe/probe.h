/* TEST INFRASTRUCTURE — C-ABI of adypt_amd/libadypt_probe.so: the device helpers of csrc/device (canon_math.hpp, shade.hpp, noise.hpp), one
 * entry per helper, so that tests/test_gpu_device_probes.py can hold each of them against the oracle's piece (oracle/oracle.cpp: orc_*) and
 * against truths that need neither side; and, at the end, the denoiser's kernels on images a test makes.  The product never links, loads or calls
 * this library.
 *
 * Every entry of the helpers: host pointers in and out, n elements (0 <= n <= 2^24).  It allocates, copies in, launches ONE grid of 256-thread workgroups
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

/* ---- The denoiser's kernels (csrc/device/denoise_kernels.hpp, the header denoise.hip compiles), one entry per kernel, each launched ONCE with the
 * grid and workgroup of the header's *_launch function, which denoise.hip launches it with too; tests/test_gpu_denoise_probes.py.
 * Images are row-major, width x height (1..4096 each) float4 per pixel unless said otherwise: X0 = (D.rgb, V), X1 = (N.xyz, hit), X2 = (P.xyz, n),
 * XA = (A.rgb, .).  Block-major arrays hold 1024 elements per block of `blocks` (n_blocks entries, 1..4096, each a block of the picture's grid of
 * 32 x 32 blocks, in any order; anything else is refused with -1): float4 per local pixel, `moments` float2, `hits` the primary-hit float4 whose .x
 * holds the triangle index as bits.  Every output is filled with the word 0x7fc0dead (a quiet NaN) before the launch: what no thread wrote keeps it. */
int adypt_probe_denoise_prepare(const float *accum, const float *moments, const float *albedo, const float *normal, const float *position, const float *hits, const int32_t *blocks,
                                const int32_t *block_spp, int n_blocks, int width, int height, float *x0, float *x1, float *x2, float *xa);
/* k_atrous<last != 0>, 1 <= step <= 64: out is the next X0, or with `last` the width x height x 3 result */
int adypt_probe_atrous(const float *x0, const float *x1, const float *x2, const float *xa, int width, int height, int step, float sigma_l, float sigma_z, int last, float *out);
/* k_rectify_window<radius>, radius 1..3; origin: the current camera's, 3 floats */
int adypt_probe_rectify_window(int radius, const float *x0, const float *x1, const float *x2, const float *xa, int width, int height, const float *origin, float *r0, float *r1);
/* k_temporal_merge<motion != 0, rectify != 0>.  The history H0 H1 H2 HA and whether there is one (`have`), its raw camera (origin 3, inv_proj 16,
 * inv_view 16 floats: temporal_camera is called here); xp, xn looked at only with motion, r0, r1, gamma and kept only with rectify (null otherwise).
 * Out: merged, X2 as the kernel leaves it (n_out in .w; not pre-filled: the kernel updates it in place), length and kept (one float per pixel). */
int adypt_probe_temporal_merge(int motion, int rectify, const float *x0, const float *x1, const float *x2, const float *xa, const float *h0, const float *h1, const float *h2, const float *ha,
                               int have, const float *origin, const float *inv_proj, const float *inv_view, float history_cap, const float *xp, const float *xn, const float *r0,
                               const float *r1, float gamma, int width, int height, float *merged, float *x2_out, float *length, float *kept);
/* k_temporal_merge_virtual (the merge by the virtual point: temporal.hpp temporal_merge_virtual).  X1.w and H1.w hold classes, xv = (Pv.xyz, len).  Out as
 * above, and counts: the two sums the host makes of the kernel's counters — pixels of class >= 2, and those of them that took history. */
int adypt_probe_temporal_merge_virtual(const float *x0, const float *x1, const float *x2, const float *xa, const float *xv, const float *h0, const float *h1, const float *h2, const float *ha,
                                       int have, const float *origin, const float *inv_proj, const float *inv_view, float history_cap, int width, int height, float *merged, float *x2_out,
                                       float *length, uint64_t *counts);
/* k_denoise_prepare_class, _moments and _virtual: adypt_probe_denoise_prepare's arguments behind which of the three.  hits.w holds the class word for the
 * class and virtual instances; g_virtual (block-major) and xv (an image, pre-filled like the others) are looked at by the virtual instance only and
 * may be null for the other two. */
enum { ADYPT_PROBE_PREPARE_CLASS = 0, ADYPT_PROBE_PREPARE_MOMENTS = 1, ADYPT_PROBE_PREPARE_VIRTUAL = 2 };
int adypt_probe_denoise_prepare_instance(int instance, const float *accum, const float *moments, const float *albedo, const float *normal, const float *position, const float *hits,
                                         const int32_t *blocks, const int32_t *block_spp, int n_blocks, int width, int height, float *x0, float *x1, float *x2, float *xa,
                                         const float *g_virtual, float *xv);
/* k_temporal_merge_moments<motion != 0>: adypt_probe_temporal_merge's arguments without the rectified call's; the fourth channel of X0, H0 and merged
 * is the raw second moment S. */
int adypt_probe_temporal_merge_moments(int motion, const float *x0, const float *x1, const float *x2, const float *xa, const float *h0, const float *h1, const float *h2, const float *ha,
                                       int have, const float *origin, const float *inv_proj, const float *inv_view, float history_cap, const float *xp, const float *xn, int width,
                                       int height, float *merged, float *x2_out, float *length);
/* k_moments_variance on the merged images (merged = (D.rgb, S), X2.w = n_out); origin: the current camera's, 3 floats.  Out: `out` = (D.rgb, V), the
 * variance read-out (one float per pixel), and the sum the host makes of the kernel's 64 count slots (zeroed before the launch). */
int adypt_probe_moments_variance(const float *merged, const float *x1, const float *x2, const float *xa, int width, int height, const float *origin, float *out, float *variance,
                                 uint64_t *spatial_count);
/* k_motion_gather.  snapshot: n_known elements of 5 float4; records: n_records >= n_known elements of tri_float4 (5..64) float4.  Both tables lie on
 * the device between 64 triangles of slack filled with 12345.0f, so that an index guard that fails shows as wrong words; a hit word outside
 * [-32, n_known + 32) is refused with -1. */
int adypt_probe_motion_gather(const float *hits, const float *normal, const float *position, const int32_t *blocks, int n_blocks, int width, int height, const float *snapshot,
                              int64_t n_known, const float *records, int64_t n_records, int tri_float4, float *xp, float *xn);
/* k_motion_snapshot: n_tris (1..2^20) records of tri_float4 float4 -> n_tris elements of 5 float4 */
int adypt_probe_motion_snapshot(const float *records, int tri_float4, int64_t n_tris, float *snapshot);
/* ---- The chain through mirrors and glass: k_chain_start<unfold != 0> and k_chain_step<unfold != 0>, one launch each.
 * The scene: n_tris (1..2^20) device triangle records of 8 float4 and n_mats (1..4096) device material records of 5 float4 (the reference's 64 bytes
 * and (texel offset, w, h, 0) of the diffuse texture); at most one texture, tex_rgb (w x h RGB8, laid out as adypt_probe_sample_texture lays it out) or
 * null for none: a material whose diffuse-texture word is 0 must describe it as (0, w, h).  Both tables lie on the device between 64 records of slack
 * filled with 12345.0f.  Refused with -1: a hit word (the bits of a hit's .x) outside [-32, n_tris + 32) other than INT32_MAX, a triangle's material id
 * outside [-32, n_mats + 32), bounces outside 1..8, segments outside 1..64, seg_cap outside 1..2^20.
 * A queue is segments x seg_cap slots of o = (origin, tmin) and d = (direction, the local pixel as bits); its counters lie 16 words apart:
 * count[16 s] of segment s, every other word stays 0.  counts: rays, followed, escaped, truncated (the kernel's ChainCounts, zero before the launch). */
/* k_chain_start over the block list (1..64 blocks): the block-major guides (float4 per local pixel; hits.x the hit word, .y .z = u v) are updated in
 * place — the kernel writes nothing but the class into hits.w of the pixels it does not follow.  Out, each pre-filled with 0x7fc0dead: state (2 float4
 * per local pixel) and the queue's o and d; queue_count (segments x 16 words) starts at 0. */
int adypt_probe_chain_start(int unfold, const float *triangles, int64_t n_tris, const float *materials, int n_mats, const uint8_t *tex_rgb, int tex_w, int tex_h, float *albedo,
                            float *normal, float *position, float *hits, const int32_t *blocks, int n_blocks, int width, int height, const float *origin, float tmin, int bounces,
                            int segments, uint32_t seg_cap, float *state, float *queue_o, float *queue_d, uint32_t *queue_count, uint64_t *counts);
/* k_chain_step over the queue (in_o, in_d, in_count) the traversal answered with in_hit (float4 per slot: the hit word as bits, u, v, t), launched with
 * chain_step_launch(segments, seg_cap).  n_px (1..2^22): the local pixels the guides (float4 each), the state (2 float4 each) and, with unfold, virt
 * (float4 each) hold; all are updated in place and lie on the device between 64 elements of slack: a word of the slack that changed is answered with
 * -10001.  Every slot's pixel word (the bits of in_d's .w) must lie in [-32, n_px + 32) or be INT32_MAX, every slot's hit word as above.  out_o and out_d
 * are pre-filled with 0x7fc0dead, out_count starts at 0.  virt and origin (the camera's, 3 floats) are looked at with unfold only. */
int adypt_probe_chain_step(int unfold, const float *triangles, int64_t n_tris, const float *materials, int n_mats, const uint8_t *tex_rgb, int tex_w, int tex_h, float *albedo,
                           float *normal, float *position, float *hits, int n_px, int segments, uint32_t seg_cap, const float *in_o, const float *in_d, const float *in_hit,
                           const uint32_t *in_count, int bounces, float tmin, float *state, float *out_o, float *out_d, uint32_t *out_count, uint64_t *counts, float *virt,
                           const float *origin);

#ifdef __cplusplus
}
#endif
#endif
