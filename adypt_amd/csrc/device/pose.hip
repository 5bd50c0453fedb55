// Posing on the device (include/adypt_hip.h adypt_bind_parts, adypt_bind_skin, adypt_pose ...; the definition: pose.hpp).  A translation unit of its
// own: nothing here is part of the tracer's code object.  A bind keeps, per context, words 0..17 of every triangle record as they are then — the rest
// pose — and the binding: one part per triangle, or four weighted joints per vertex.  What one adypt_pose runs, all on the context's stream after the
// context has been drained:
//     the staging copy   n_matrices x 48 bytes: all that comes from the host
//     k_pose             one thread per triangle: rest pose + binding + matrices -> words 0..17 of the record (positions, normals).  A pose never reads
//                        the records, so poses do not compound.  The rest pose and the binding are kept in planes — plane k holds the k-th 16 bytes of
//                        every triangle — so a wave's loads are 16 bytes per lane (8 for the last plane of the rest pose and for the joints),
//                        neighbouring lanes neighbouring addresses; a matrix is three 16-byte loads from an array that stays in the caches.  The record
//                        is written as adypt_update_triangles' k_refit_scatter writes it: four 16-byte stores and one of 8 bytes for words 16 and 17,
//                        which share their 16 bytes with the material id and the class word.  Every array of a lane is indexed by constants after
//                        unrolling: registers, no scratch.  With a morph layer (adypt_bind_morph) the MORPHED instantiations put the morph stage
//                        between the rest pose's loads and the matrices: a lane reads its two offsets and loops over its entries, which the bind has
//                        sorted by (triangle, target); per entry the target index and the weight, and the 72 bytes of deltas — planes like the rest
//                        pose's — only where the weight is not 0.  The weights (4 B per target) are staged beside the matrices.
//     (refit.hip)        the refit's tail, refit_tail: per-reference copy, Woop data, node levels, root card, reset
#include "ctx_unit.hpp"
#include "pose.hpp"
#include "pose_internal.hpp"
#include "refit_internal.hpp"
#include "tri_record.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

#include <string>
#include <vector>

using namespace adypt;

namespace {

constexpr int kPoseThreads = 256;
constexpr int kRestPlanes = 4;                              // float4 planes of the rest pose: words 0..15; words 16, 17 are a float2 plane
constexpr int kMatrixVecs = kPoseMatrixFloats / 4;          // a matrix is three float4
static_assert(kTriRecordWords == 32 && kPoseSlots == 4, "the record of tri_record.hpp; a vertex's slots are one float4 of weights and one uint2 of joints");

// words 0..17 of every record into the planes: once per bind
__global__ __launch_bounds__(kPoseThreads) void k_pose_capture(const float4 *__restrict__ records, int tri_float4, int64_t n, float4 *__restrict__ rest4, float2 *__restrict__ rest2)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const float4 *rec = records + (size_t)i * (size_t)tri_float4;
	for(int k = 0; k < kRestPlanes; ++k) rest4[(size_t)k * (size_t)n + (size_t)i] = rec[k];
	rest2[i] = ((const float2 *)rec)[8];
}

__device__ __forceinline__ void load_matrix(const float4 *__restrict__ mats, uint32_t j, float B[kPoseMatrixFloats])
{
	const float4 *m = mats + (size_t)j * kMatrixVecs;
	const float4 r0 = m[0], r1 = m[1], r2 = m[2];
	B[0] = r0.x; B[1] = r0.y; B[2] = r0.z; B[3] = r0.w; B[4] = r1.x; B[5] = r1.y; B[6] = r1.z; B[7] = r1.w; B[8] = r2.x; B[9] = r2.y; B[10] = r2.z; B[11] = r2.w;
}

// parts: n part indices (SKINNED: unused); joints, weights: three planes of n — vertex v's four joints as 16-bit halves of a uint2, its four weights as
// a float4 (!SKINNED: unused); mats: n_matrices x 3 float4.  Every index has been checked on the host (pose.hpp, pose_refuse_*).
// The morph layer as the kernel reads it (MORPHED; otherwise unused): offsets — n + 1 places into the entries, which are sorted by (triangle, target);
// target — the entry's target index; d4, d2 — the entry's 18 deltas in four float4 planes and one float2 plane of n_entries; w — one weight per target.
struct MorphView {
	const int32_t *__restrict__ offsets;
	const int32_t *__restrict__ target;
	const float4 *__restrict__ d4;
	const float2 *__restrict__ d2;
	const float *__restrict__ w;
	int64_t n_entries;
};

template <bool SKINNED, bool MORPHED>
__global__ __launch_bounds__(kPoseThreads) void k_pose(float4 *records, int tri_float4, int64_t n, const float4 *__restrict__ rest4, const float2 *__restrict__ rest2,
                                                       const int32_t *__restrict__ parts, const uint2 *__restrict__ joints, const float4 *__restrict__ weights,
                                                       const float4 *__restrict__ mats, const MorphView morph)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const size_t at = (size_t)i, plane = (size_t)n;
	const float4 a = rest4[at], b = rest4[plane + at], c = rest4[2 * plane + at], d = rest4[3 * plane + at];
	const float2 e = rest2[at];
	float in[18] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y};
	if(MORPHED)
	{
		// the lane's entries in ascending target index: a variable trip count; the index and the weight first, the 72 bytes of deltas only where the
		// weight is not 0.  `in` is indexed by constants only (pose_morph unrolls): registers
		const size_t eplane = (size_t)morph.n_entries;
		const int32_t end = morph.offsets[at + 1];
		for(int32_t k = morph.offsets[at]; k < end; ++k)
		{
			const float w = morph.w[(uint32_t)morph.target[k]];
			if(w == 0.0f) continue;
			const size_t ek = (size_t)k;
			const float4 da = morph.d4[ek], db = morph.d4[eplane + ek], dc = morph.d4[2 * eplane + ek], dd = morph.d4[3 * eplane + ek];
			const float2 de = morph.d2[ek];
			const float delta[kMorphWords] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w, dc.x, dc.y, dc.z, dc.w, dd.x, dd.y, dd.z, dd.w, de.x, de.y};
			pose_morph(in, w, delta);
		}
	}
	float out[18];
	float M[kPoseMatrixFloats];
	if(!SKINNED) load_matrix(mats, (uint32_t)parts[at], M);
#pragma unroll
	for(int v = 0; v < 3; ++v)
	{
		if(SKINNED)
		{
			const uint2 jj = joints[(size_t)v * plane + at];
			const float4 ww = weights[(size_t)v * plane + at];
			const uint32_t j[kPoseSlots] = {jj.x & 0xffffu, jj.x >> 16, jj.y & 0xffffu, jj.y >> 16};
			const float w[kPoseSlots] = {ww.x, ww.y, ww.z, ww.w};
			bool first = true;
#pragma unroll
			for(int k = 0; k < kPoseMatrixFloats; ++k) M[k] = 0.0f;
#pragma unroll
			for(int k = 0; k < kPoseSlots; ++k)
			{
				if(w[k] == 0.0f) continue; // (the slot's joint index is never read as an index)
				float B[kPoseMatrixFloats];
				load_matrix(mats, j[k], B);
				pose_weigh(M, first, w[k], B);
				first = false;
			}
		}
		pose_vertex(M, in + 3 * v, in + 9 + 3 * v, out + 3 * v, out + 9 + 3 * v);
	}
	float4 *rec = records + at * (size_t)tri_float4;
	rec[0] = make_float4(out[0], out[1], out[2], out[3]);
	rec[1] = make_float4(out[4], out[5], out[6], out[7]);
	rec[2] = make_float4(out[8], out[9], out[10], out[11]);
	rec[3] = make_float4(out[12], out[13], out[14], out[15]);
	((float2 *)rec)[8] = make_float2(out[16], out[17]); // (words 18, 19 — material id, class word — share this vector and keep their bytes)
}

// what adypt_bind_morph leaves on the device, the entries sorted by (triangle, target)
struct Layer {
	int32_t n_targets = 0;
	int64_t n_entries = 0, n_tris_touched = 0;
	Buffer<float4> d4;        // 4 planes of n_entries: 64 B per entry
	Buffer<float2> d2;        // 8 B per entry
	Buffer<int32_t> target;   // 4 B per entry
	Buffer<int32_t> offsets;  // n_tris + 1
	Buffer<float> w;          // the staging buffer of the weights: 4 B per target
	int64_t device_bytes() const { return (int64_t)(d4.bytes() + d2.bytes() + target.bytes() + offsets.bytes() + w.bytes()); }
	MorphView view() const { return MorphView{offsets.get(), target.get(), d4.get(), d2.get(), w.get(), n_entries}; }
};

// what a bind leaves on the device
struct Binding {
	int32_t kind = kPoseNone, n_matrices = 0;
	int64_t n_tris = 0;
	Layer layer;              // goes with the binding: its deltas are of this rest pose
	Buffer<float4> rest4;     // 4 planes of n_tris: 64 B per triangle
	Buffer<float2> rest2;     // 8 B per triangle
	Buffer<int32_t> parts;    // parts: 4 B per triangle
	Buffer<uint2> joints;     // skin: 3 planes of n_tris, 24 B per triangle
	Buffer<float4> weights;   // skin: 3 planes of n_tris, 48 B per triangle
	Buffer<float4> mats;      // the staging buffer of the matrices: 48 B each
	int64_t device_bytes() const { return (int64_t)(rest4.bytes() + rest2.bytes() + parts.bytes() + joints.bytes() + weights.bytes() + mats.bytes()); }
};

// kept per context
struct Poser {
	Binding bound;
};

// The binding `kind` of the context's triangles as they are now; everything has been checked.  The new binding is complete before it takes the place
// of the old one: a failure leaves the old one in place.
int bind(adypt_ctx *c, const char *who, int32_t kind, const int32_t *parts, const uint16_t *joints, const float *weights, int64_t n, int32_t n_matrices)
{
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	const CtxScene sc = ctx_scene(c);
	if(sc.tri_float4 * 4 != kTriRecordWords) return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": the record layout is not tri_record.hpp's");
	Binding nb;
	nb.kind = kind; nb.n_matrices = n_matrices; nb.n_tris = n;
	CTX_TRY(c, at_least(nb.rest4, (size_t)n * kRestPlanes));
	CTX_TRY(c, at_least(nb.rest2, (size_t)n));
	CTX_TRY(c, at_least(nb.mats, (size_t)n_matrices * kMatrixVecs));
	std::vector<uint2> h_joints;
	std::vector<float4> h_weights;
	if(kind == kPoseParts)
	{
		CTX_TRY(c, at_least(nb.parts, (size_t)n));
		CTX_TRY(c, hipMemcpyAsync(nb.parts.get(), parts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	}
	else
	{
		CTX_TRY(c, at_least(nb.joints, (size_t)n * 3));
		CTX_TRY(c, at_least(nb.weights, (size_t)n * 3));
		h_joints.resize((size_t)n * 3);
		h_weights.resize((size_t)n * 3);
		for(int64_t t = 0; t < n; ++t)
			for(int v = 0; v < 3; ++v)
			{
				const uint16_t *j = joints + (size_t)t * kPoseTriSlots + v * kPoseSlots;
				const float *w = weights + (size_t)t * kPoseTriSlots + v * kPoseSlots;
				h_joints[(size_t)v * (size_t)n + (size_t)t] = make_uint2((uint32_t)j[0] | (uint32_t)j[1] << 16, (uint32_t)j[2] | (uint32_t)j[3] << 16);
				h_weights[(size_t)v * (size_t)n + (size_t)t] = make_float4(w[0], w[1], w[2], w[3]);
			}
		CTX_TRY(c, hipMemcpyAsync(nb.joints.get(), h_joints.data(), h_joints.size() * sizeof(uint2), hipMemcpyHostToDevice, i.stream));
		CTX_TRY(c, hipMemcpyAsync(nb.weights.get(), h_weights.data(), h_weights.size() * sizeof(float4), hipMemcpyHostToDevice, i.stream));
	}
	hipLaunchKernelGGL(k_pose_capture, dim3(grid_of(n, kPoseThreads)), dim3(kPoseThreads), 0, i.stream, (const float4 *)sc.triangles, sc.tri_float4, n, nb.rest4.get(), nb.rest2.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	ctx_state<Poser>(c, kAttachPose)->bound = std::move(nb); // (the old binding's memory goes with `nb`)
	return ADYPT_OK;
}

// the refit whose writer is k_pose
template <bool SKINNED, bool MORPHED> void launch_pose(const CtxInfo &i, const CtxScene &sc, const Binding &b)
{
	hipLaunchKernelGGL((k_pose<SKINNED, MORPHED>), dim3(grid_of(b.n_tris, kPoseThreads)), dim3(kPoseThreads), 0, i.stream, sc.triangles, sc.tri_float4, b.n_tris,
	                   (const float4 *)b.rest4.get(), (const float2 *)b.rest2.get(), (const int32_t *)b.parts.get(), (const uint2 *)b.joints.get(), (const float4 *)b.weights.get(),
	                   (const float4 *)b.mats.get(), b.layer.view());
}

// the refit whose writer is k_pose; morph_weights: the layer's n_targets weights, or null for all 0 (looked at only where there is a layer)
int pose_and_refit(adypt_ctx *c, const Binding &b, const float *matrices, const float *morph_weights)
{
	CTX_STEP(refit_begin(c));
	const CtxInfo i = ctx_info(c);
	const CtxScene sc = ctx_scene(c);
	const bool morphed = b.layer.n_targets > 0, skinned = b.kind == kPoseSkin;
	CTX_TRY(c, hipMemcpyAsync(b.mats.get(), matrices, (size_t)b.n_matrices * kPoseMatrixFloats * sizeof(float), hipMemcpyHostToDevice, i.stream));
	if(morphed && morph_weights) CTX_TRY(c, hipMemcpyAsync(b.layer.w.get(), morph_weights, (size_t)b.layer.n_targets * sizeof(float), hipMemcpyHostToDevice, i.stream));
	if(morphed && !morph_weights) CTX_TRY(c, hipMemsetAsync(b.layer.w.get(), 0, (size_t)b.layer.n_targets * sizeof(float), i.stream));
	if(morphed) skinned ? launch_pose<true, true>(i, sc, b) : launch_pose<false, true>(i, sc, b);
	else skinned ? launch_pose<true, false>(i, sc, b) : launch_pose<false, false>(i, sc, b);
	CTX_TRY(c, hipGetLastError());
	return refit_tail(c);
}

// what both binds refuse before the device is touched: the reason, or empty
std::string bind_refused(adypt_ctx *c, const char *who, bool have_arrays, int64_t n_tris, int64_t n_matrices, const char *what)
{
	const std::string w = std::string(who) + ": ";
	if(!have_arrays) return w + "null argument";
	const int64_t have = ctx_scene(c).n_tris;
	if(n_tris != have) return w + "n_tris is " + std::to_string(n_tris) + ", the context holds " + std::to_string(have) + " triangles";
	if(pose_refuse_count(n_matrices)) return w + "the number of " + what + " must be in [1, 65536]";
	return std::string();
}

// adypt_pose and adypt_pose_morph: morph_weights null with n_targets 0 is every weight 0
int pose(adypt_ctx *c, const char *who, const float *matrices, int32_t n_matrices, const float *morph_weights, int32_t n_targets, const adypt_bvh_params *params,
         const adypt_pose_policy *policy, adypt_pose_outcome *outcome)
{
	if(!c) return ADYPT_E_INVALID;
	if(!matrices) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": matrices is null");
	if(!morph_weights && n_targets != 0) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": morph_weights is null");
	const Poser *ps = ctx_state_if_any<Poser>(c, kAttachPose);
	if(!ps || ps->bound.kind == kPoseNone) return ctx_fail(c, ADYPT_E_STATE, std::string(who) + ": no binding (adypt_bind_parts, adypt_bind_skin; adypt_set_triangles drops it)");
	const Binding &b = ps->bound;
	if(b.n_tris != ctx_scene(c).n_tris) return ctx_fail(c, ADYPT_E_STATE, std::string(who) + ": the binding is not of the context's triangles");
	if(n_matrices != b.n_matrices) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": n_matrices is " + std::to_string(n_matrices) + ", the binding has " + std::to_string(b.n_matrices));
	if(const char *r = pose_refuse_matrices(matrices, n_matrices)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": " + r);
	if(morph_weights || n_targets != 0)
		if(const char *r = pose_refuse_morph_weights(morph_weights, n_targets, b.layer.n_targets)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": " + r);
	if(!policy)
	{
		CTX_TRY(c, hipSetDevice(ctx_info(c).device));
		CTX_STEP(pose_and_refit(c, b, matrices, morph_weights));
		if(outcome) *outcome = adypt_pose_outcome{};
		return ADYPT_OK;
	}
	BuildRequest request;
	if(const char *why = refit_policy_refused(params, policy, &request)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": " + why);
	return refit_under_policy(c, who, request, policy->rebuild_above, outcome, [&]() { return pose_and_refit(c, b, matrices, morph_weights); });
}

}  // namespace

namespace adypt {

void pose_drop_binding(adypt_ctx *c)
{
	Poser *ps = ctx_state_if_any<Poser>(c, kAttachPose);
	if(ps) ps->bound = Binding();
}

}  // namespace adypt

extern "C" {

int adypt_bind_parts(adypt_ctx *c, const int32_t *part_of_triangle, int64_t n_tris, int32_t n_parts)
{
	if(!c) return ADYPT_E_INVALID;
	const char *who = "adypt_bind_parts";
	std::string why = bind_refused(c, who, part_of_triangle != nullptr, n_tris, n_parts, "parts");
	if(why.empty())
		if(const char *r = pose_refuse_parts(part_of_triangle, n_tris, n_parts)) why = std::string(who) + ": " + r;
	if(!why.empty()) return ctx_fail(c, ADYPT_E_INVALID, why);
	return bind(c, who, kPoseParts, part_of_triangle, nullptr, nullptr, n_tris, n_parts);
}

int adypt_bind_skin(adypt_ctx *c, const uint16_t *joints, const float *weights, int64_t n_tris, int32_t n_joints)
{
	if(!c) return ADYPT_E_INVALID;
	const char *who = "adypt_bind_skin";
	std::string why = bind_refused(c, who, joints && weights, n_tris, n_joints, "joints");
	if(why.empty())
		if(const char *r = pose_refuse_skin(joints, weights, n_tris, n_joints)) why = std::string(who) + ": " + r;
	if(!why.empty()) return ctx_fail(c, ADYPT_E_INVALID, why);
	return bind(c, who, kPoseSkin, nullptr, joints, weights, n_tris, n_joints);
}

int adypt_pose(adypt_ctx *c, const float *matrices, int32_t n_matrices, const adypt_bvh_params *params, const adypt_pose_policy *policy, adypt_pose_outcome *outcome)
{
	return pose(c, "adypt_pose", matrices, n_matrices, nullptr, 0, params, policy, outcome);
}

int adypt_pose_morph(adypt_ctx *c, const float *matrices, int32_t n_matrices, const float *morph_weights, int32_t n_targets, const adypt_bvh_params *params,
                     const adypt_pose_policy *policy, adypt_pose_outcome *outcome)
{
	return pose(c, "adypt_pose_morph", matrices, n_matrices, morph_weights, n_targets, params, policy, outcome);
}

int adypt_bind_morph(adypt_ctx *c, const int32_t *triangle_of_entry, const int32_t *target_of_entry, const float *deltas, int64_t n_entries, int32_t n_targets)
{
	if(!c) return ADYPT_E_INVALID;
	const std::string who = "adypt_bind_morph: ";
	if(!triangle_of_entry || !target_of_entry || !deltas) return ctx_fail(c, ADYPT_E_INVALID, who + "null argument");
	Poser *ps = ctx_state_if_any<Poser>(c, kAttachPose);
	if(!ps || ps->bound.kind == kPoseNone || ps->bound.n_tris != ctx_scene(c).n_tris)
		return ctx_fail(c, ADYPT_E_STATE, who + "no binding to add the layer to (adypt_bind_parts, adypt_bind_skin)");
	const int64_t n = ps->bound.n_tris;
	std::vector<int32_t> order, offsets;
	const char *r = pose_refuse_morph_counts(n_entries, n_targets);
	if(!r) r = pose_refuse_morph_entries(triangle_of_entry, target_of_entry, deltas, n_entries, n, n_targets);
	if(!r) r = pose_morph_order(triangle_of_entry, target_of_entry, n_entries, n, order, offsets);
	if(r) return ctx_fail(c, ADYPT_E_INVALID, who + r);
	// the entries in their order, in planes
	const size_t ne = (size_t)n_entries;
	std::vector<float4> h_d4(ne * kRestPlanes);
	std::vector<float2> h_d2(ne);
	std::vector<int32_t> h_target(ne);
	for(size_t k = 0; k < ne; ++k)
	{
		const float *d = deltas + (size_t)order[k] * kMorphWords;
		for(int q = 0; q < kRestPlanes; ++q) h_d4[(size_t)q * ne + k] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
		h_d2[k] = make_float2(d[16], d[17]);
		h_target[k] = target_of_entry[order[k]];
	}
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	Layer nl;
	nl.n_targets = n_targets; nl.n_entries = n_entries;
	for(int64_t t = 0; t < n; ++t) nl.n_tris_touched += offsets[(size_t)t + 1] > offsets[(size_t)t];
	CTX_TRY(c, at_least(nl.d4, h_d4.size()));
	CTX_TRY(c, at_least(nl.d2, ne));
	CTX_TRY(c, at_least(nl.target, ne));
	CTX_TRY(c, at_least(nl.offsets, offsets.size()));
	CTX_TRY(c, at_least(nl.w, (size_t)n_targets));
	CTX_TRY(c, hipMemcpyAsync(nl.d4.get(), h_d4.data(), h_d4.size() * sizeof(float4), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipMemcpyAsync(nl.d2.get(), h_d2.data(), ne * sizeof(float2), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipMemcpyAsync(nl.target.get(), h_target.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipMemcpyAsync(nl.offsets.get(), offsets.data(), offsets.size() * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	ps->bound.layer = std::move(nl); // (complete: the old layer's memory goes with `nl`)
	return ADYPT_OK;
}

int adypt_unbind_morph(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	CTX_TRY(c, hipSetDevice(ctx_info(c).device));
	CTX_STEP(ctx_drain(c));
	Poser *ps = ctx_state_if_any<Poser>(c, kAttachPose);
	if(ps) ps->bound.layer = Layer();
	return ADYPT_OK;
}

int adypt_get_morph_binding(adypt_ctx *c, adypt_morph_binding *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, "adypt_get_morph_binding: out is null");
	const Poser *ps = ctx_state_if_any<Poser>(c, kAttachPose);
	*out = adypt_morph_binding{};
	if(ps && ps->bound.layer.n_targets > 0)
	{
		const Layer &l = ps->bound.layer;
		out->n_targets = l.n_targets; out->n_entries = l.n_entries; out->n_tris_touched = l.n_tris_touched; out->device_bytes = l.device_bytes();
	}
	return ADYPT_OK;
}

int adypt_multi_bind_morph(adypt_multi *m, const int32_t *triangle_of_entry, const int32_t *target_of_entry, const float *deltas, int64_t n_entries, int32_t n_targets)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_bind_morph(c, triangle_of_entry, target_of_entry, deltas, n_entries, n_targets); });
}

int adypt_multi_pose_morph(adypt_multi *m, const float *matrices, int32_t n_matrices, const float *morph_weights, int32_t n_targets, const adypt_bvh_params *params,
                           const adypt_pose_policy *policy, adypt_pose_outcome *outcome)
{
	return multi_each_outcome(m, "adypt_multi_pose_morph", outcome,
	                          [=](adypt_ctx *c, adypt_pose_outcome *o) { return adypt_pose_morph(c, matrices, n_matrices, morph_weights, n_targets, params, policy, o); });
}

int adypt_multi_unbind_morph(adypt_multi *m)
{
	return multi_each(m, [](adypt_ctx *c) { return adypt_unbind_morph(c); });
}

// every device holds the same layer: the first one's
int adypt_multi_get_morph_binding(adypt_multi *m, adypt_morph_binding *out)
{
	if(m && !out) { multi_set_error(m, "adypt_multi_get_morph_binding: out is null"); return ADYPT_E_INVALID; }
	int k = 0;
	return multi_each(m, [&](adypt_ctx *c) {
		adypt_morph_binding b{};
		CTX_STEP(adypt_get_morph_binding(c, &b));
		if(k++ == 0) *out = b;
		return (int)ADYPT_OK;
	});
}

int adypt_unbind_pose(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	CTX_TRY(c, hipSetDevice(ctx_info(c).device));
	CTX_STEP(ctx_drain(c));
	pose_drop_binding(c);
	return ADYPT_OK;
}

int adypt_get_pose_binding(adypt_ctx *c, adypt_pose_binding *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, "adypt_get_pose_binding: out is null");
	const Poser *ps = ctx_state_if_any<Poser>(c, kAttachPose);
	*out = adypt_pose_binding{};
	if(ps) *out = adypt_pose_binding{ps->bound.kind, ps->bound.n_matrices, ps->bound.n_tris, ps->bound.device_bytes()};
	return ADYPT_OK;
}

// the scene is replicated: the same binding and the same pose on every device
int adypt_multi_bind_parts(adypt_multi *m, const int32_t *part_of_triangle, int64_t n_tris, int32_t n_parts)
{
	// (bad arguments are refused by the first context: none has changed)
	return multi_each(m, [=](adypt_ctx *c) { return adypt_bind_parts(c, part_of_triangle, n_tris, n_parts); });
}

int adypt_multi_bind_skin(adypt_multi *m, const uint16_t *joints, const float *weights, int64_t n_tris, int32_t n_joints)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_bind_skin(c, joints, weights, n_tris, n_joints); });
}

int adypt_multi_pose(adypt_multi *m, const float *matrices, int32_t n_matrices, const adypt_bvh_params *params, const adypt_pose_policy *policy, adypt_pose_outcome *outcome)
{
	return multi_each_outcome(m, "adypt_multi_pose", outcome, [=](adypt_ctx *c, adypt_pose_outcome *o) { return adypt_pose(c, matrices, n_matrices, params, policy, o); });
}

int adypt_multi_unbind_pose(adypt_multi *m)
{
	return multi_each(m, [](adypt_ctx *c) { return adypt_unbind_pose(c); });
}

// every device holds the same binding: the first one's
int adypt_multi_get_pose_binding(adypt_multi *m, adypt_pose_binding *out)
{
	if(m && !out) { multi_set_error(m, "adypt_multi_get_pose_binding: out is null"); return ADYPT_E_INVALID; }
	int k = 0;
	return multi_each(m, [&](adypt_ctx *c) {
		adypt_pose_binding b{};
		CTX_STEP(adypt_get_pose_binding(c, &b));
		if(k++ == 0) *out = b;
		return (int)ADYPT_OK;
	});
}

}  // extern "C"
