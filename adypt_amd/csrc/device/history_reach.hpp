// History-aware sampling: how much history a pixel WILL find in the temporal merge, known before the first sample of a pose is traced, and the sample
// count every 32 x 32 block needs on top of it (adypt_plan_by_history, adypt_trace_by_history; the kernel and the host side: history_plan.hip).
// THE definition for host and device (no HIP needed: tests/test_history_reach_definition.py compiles it on the host with -ffp-contract=off).  The
// arithmetic rules are temporal.hpp's: binary32, the operations in the order written, NO fma, every comparison written so that a NaN yields "no
// history".  The integer part (the bins, the plan, the order of work) is exact.
//
// The merge's acceptance rule is a pure function of the guides, the history and its camera: the call's own sample count n does not enter the length
// nh = min(sum w n_q / sum w, history_cap) that temporal_merge_through<false, false> blends with, and its out.n is n + nh.  history_reach is that nh,
// by the same reprojection, the same four taps, the same tests and the same weights, without the colour sums — so it can be asked at 0 spp, from the
// guides ctx_capture_guides leaves.  Not covered: a rectified call shortens the length by a share that depends on samples not yet traced (the plan
// may overestimate there), and the merge by the virtual point has a rule of its own.
#pragma once
#include "temporal.hpp"

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace adypt {

// The length the merge of this pixel will take from the history; 0 wherever temporal_merge_through<false, false> returns early.  (n, p): the normal and
// the point the taps are held against and that is reprojected — the current ones where the surface stands still, temporal_previous_point's for the
// motion form (history_reach_motion).  ca: the albedo as captured.  h0 is read for its finiteness test only.
template <class Hist>
ADYPT_HOST_DEVICE float history_reach(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, bool hit, float nx, float ny, float nz, float px, float py, float pz,
                                      const Dn4 &ca, float history_cap)
{
	if(!have || !hit) return 0.0f;
	float fx, fy, dist;
	if(!temporal_reproject(cam, width, height, px, py, pz, &fx, &fy, &dist)) return 0.0f;
	if(!(fx >= -1.0f && fx < (float)width && fy >= -1.0f && fy < (float)height)) return 0.0f;
	const float bx = floorf(fx), by = floorf(fy);
	const int ix = (int)bx, iy = (int)by;
	const float ux = fx - bx, uy = fy - by;
	const float tol = kTemporalPlaneTol * dist;
	float sw = 0.0f, sn = 0.0f;
	for(int ty = 0; ty <= 1; ++ty)
		for(int tx = 0; tx <= 1; ++tx)
		{
			const int qx = ix + tx, qy = iy + ty;
			if(qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
			const int q = qy * width + qx;
			const Dn4 q1 = hist.h1(q);
			if(!(q1.w != 0.0f)) continue;
			if(!((nx * q1.x + ny * q1.y) + nz * q1.z >= kTemporalNormalMin)) continue;
			const Dn4 q2 = hist.h2(q);
			const float dx = q2.x - px, dy = q2.y - py, dz = q2.z - pz;
			if(!(fabsf((nx * dx + ny * dy) + nz * dz) <= tol)) continue;
			const Dn4 qa = hist.ha(q);
			if(!(fabsf(qa.x - ca.x) <= kTemporalAlbedoTol && fabsf(qa.y - ca.y) <= kTemporalAlbedoTol && fabsf(qa.z - ca.z) <= kTemporalAlbedoTol)) continue;
			const Dn4 q0 = hist.h0(q);
			if(!(fabsf(q0.x) <= kTemporalFiniteMax && fabsf(q0.y) <= kTemporalFiniteMax && fabsf(q0.z) <= kTemporalFiniteMax && fabsf(q0.w) <= kTemporalFiniteMax &&
			     q2.w > 0.0f && q2.w <= kTemporalFiniteMax)) continue;
			const float w = (tx == 0 ? 1.0f - ux : ux) * (ty == 0 ? 1.0f - uy : uy);
			sw = sw + w;
			sn = sn + w * q2.w;
		}
	if(!(sw > kTemporalMinWeight)) return 0.0f;
	const float hq = sn / sw;
	return hq < history_cap ? hq : history_cap;
}

// The two forms by the words the merge kernels are given: c1 = (N.xyz, hit), c2 = (P.xyz, .), ca = (A.rgb, .) as denoise_prepare_pixel<false> writes
// them, and for the motion form xp, xn of temporal_previous_point (xn.w == 0: no history).
template <class Hist>
ADYPT_HOST_DEVICE float history_reach_still(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, const Dn4 &c1, const Dn4 &c2, const Dn4 &ca, float history_cap)
{
	return history_reach(hist, have, cam, width, height, c1.w != 0.0f, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z, ca, history_cap);
}
template <class Hist>
ADYPT_HOST_DEVICE float history_reach_motion(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, const Dn4 &c1, const Dn4 &ca, float history_cap, const Dn4 &xp,
                                             const Dn4 &xn)
{
	return history_reach(hist, have && xn.w != 0.0f, cam, width, height, c1.w != 0.0f, xn.x, xn.y, xn.z, xp.x, xp.y, xp.z, ca, history_cap);
}

// ---- the bins of a block ----
// Every block counts its hit pixels inside the image by the whole samples of history they will find: bin k < 64 holds the pixels with floor(L) == k,
// bin 64 those with L >= 64.  Miss pixels and pixels outside the image are in no bin; `hits` is the sum of the bins.
constexpr int kReachBins = 65;
ADYPT_HOST_DEVICE int reach_bin(float L) { return L >= 64.0f ? 64 : (int)floorf(L); } // (L is never negative or a NaN: n_q > 0 and the weights are)

// ---- the plan of a block ----
constexpr int kPlanMaxTarget = 1 << 20;
constexpr int kPlanDefaultTolerance = 31; // permille of a block's hit pixels that may stay below the target: about one row of a block

// THE argument rule of every entry
inline bool plan_args_valid(int target, int min_spp, int max_spp, int step, int tolerance_permille, float history_cap)
{
	return target >= 1 && target <= kPlanMaxTarget && min_spp >= 2 && max_spp >= min_spp && step >= 1 && tolerance_permille >= 0 && tolerance_permille <= 999 && temporal_cap_valid(history_cap);
}

// The sample count of a block from its bins: the smallest candidate n — min_spp, min_spp + step, ..., the last cut to max_spp — that leaves at most
// `allowed` = hits * tolerance_permille / 1000 hit pixels with bin + n < target; max_spp if none does, min_spp for a block without a hit pixel.
inline int plan_block(const uint32_t *bins, int target, int min_spp, int max_spp, int step, int tolerance_permille)
{
	uint64_t hits = 0;
	for(int k = 0; k < kReachBins; ++k) hits += bins[k];
	if(hits == 0) return min_spp;
	const uint64_t allowed = hits * (uint64_t)tolerance_permille / 1000u;
	for(int64_t at = min_spp;; at += step)
	{
		const int n = (int)std::min<int64_t>(at, max_spp);
		uint64_t below = 0; // the hit pixels with bin + n < target
		for(int k = 0; k < kReachBins && k + n < target; ++k) below += bins[k];
		if(below <= allowed || n == max_spp) return n;
	}
}

// is `want` one of the candidates
inline bool plan_is_candidate(int want, int min_spp, int max_spp, int step) { return want == max_spp || (want >= min_spp && want < max_spp && (want - min_spp) % step == 0); }

// ---- the order of work ----
// wants: (image block index, want) of every block of the image.  The distinct wants in ascending order: for each, `want - spp()` frames are traced,
// then the blocks of that want are frozen at it — but the blocks of the LARGEST want stay active (one set change saved; they stand at the frame counter).
// spp(): the frame counter; trace(n): n more frames of the active blocks; freeze(blocks, spp): those image blocks stop at spp frames (every device
// passes over the blocks of other owners).  The two return 0 or the code this returns.  Nothing is read back: no noise, no stepping loop.
template <class Spp, class Trace, class Freeze>
int trace_plan(const std::vector<std::pair<int32_t, int32_t>> &wants, Spp spp, Trace trace, Freeze freeze)
{
	std::vector<int32_t> distinct;
	for(const auto &bw : wants) distinct.push_back(bw.second);
	std::sort(distinct.begin(), distinct.end());
	distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
	for(size_t k = 0; k < distinct.size(); ++k)
	{
		const int want = distinct[k];
		const int n = want - spp();
		int r = n > 0 ? trace(n) : 0;
		if(r != 0) return r;
		if(k + 1 == distinct.size()) break;
		std::vector<int32_t> stop;
		for(const auto &bw : wants) if(bw.second == want) stop.push_back(bw.first);
		if((r = freeze(stop, want)) != 0) return r;
	}
	return 0;
}

}  // namespace adypt
