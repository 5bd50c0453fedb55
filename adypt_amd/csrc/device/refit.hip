// Moving geometry (include/adypt_hip.h adypt_update_triangles ...; the definition: refit.hpp, the order: refit_plan.hpp, the Woop data: woop.hpp).  A
// translation unit of its own: nothing here is part of the tracer's code object.  What one update runs, all on the context's stream after the context
// has been drained:
//     k_refit_scatter  the new positions (and normals) of triangles [first, first + count) into the device triangle records
//     (tracer.hip)     k_expand_references again, when the context keeps the per-reference copy of the records
//     k_refit_woop     one thread per reference: its triangle's Woop matrix
//     k_refit_nodes    one launch per level of the tree, deepest first: 8 lanes per node, one slot per lane.  A level reads only the exact boxes of
//                      deeper levels, which earlier launches on the same stream wrote: the stream order is the whole dependency — no atomics, no
//                      flags between workgroups, no fences.
// Everything around the scatter is refit_begin and refit_tail (refit_internal.hpp), which adypt_pose (pose.hip) runs around its own writer of the records.
// The plan (every node's level) is made once per context, at the first update, from one copy of the node array to the host; the topology never changes.
// Also here: the SAH cost of the tree as it is (tree_cost.hpp; adypt_get_tree_cost) and the refit that rebuilds when that cost says so
// (adypt_update_triangles_auto):
//     k_tree_cost      one launch over the node array, 8 lanes per node, one slot per lane: two 64-bit integer sums
#include "ctx_unit.hpp"
#include "refit_plan.hpp"
#include "refit_internal.hpp"
#include "build_internal.hpp"
#include "tree_cost.hpp"
#include "woop.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace adypt;

namespace {

constexpr int kRefitThreads = 256;
constexpr int kLanesPerNode = 8, kNodesPerGroup = kRefitThreads / kLanesPerNode; // a workgroup refits 32 nodes
constexpr int kNodeUint4 = kNodeBytes / 16;

// one thread per triangle: 9 position floats, and 9 normal floats when given, into floats 0..8 and 9..17 of the record
__global__ __launch_bounds__(kRefitThreads) void k_refit_scatter(float4 *triangles, int tri_float4, int64_t first, int64_t count, const float *positions, const float *normals)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= count) return;
	float4 *rec = triangles + (size_t)(first + i) * (size_t)tri_float4;
	const float *p = positions + (size_t)i * 9;
	rec[0] = make_float4(p[0], p[1], p[2], p[3]);
	rec[1] = make_float4(p[4], p[5], p[6], p[7]);
	if(!normals) { ((float *)rec)[8] = p[8]; return; }
	const float *n = normals + (size_t)i * 9;
	rec[2] = make_float4(p[8], n[0], n[1], n[2]);
	rec[3] = make_float4(n[3], n[4], n[5], n[6]);
	((float2 *)rec)[8] = make_float2(n[7], n[8]);
}

// one thread per reference
__global__ __launch_bounds__(kRefitThreads) void k_refit_woop(const float4 *triangles, int tri_float4, const int32_t *tri_indices, int64_t n_refs, float4 *woop)
{
	const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(r >= n_refs) return;
	const float4 *rec = triangles + (size_t)tri_indices[r] * (size_t)tri_float4;
	float p[9], o[12];
	load_positions(rec, p);
	woop_matrix(p, o);
	float4 *out = woop + (size_t)r * 3;
	out[0] = make_float4(o[0], o[1], o[2], o[3]);
	out[1] = make_float4(o[4], o[5], o[6], o[7]);
	out[2] = make_float4(o[8], o[9], o[10], o[11]);
}

// The nodes level[0 .. n_level) of one level.  Lane s of a node's 8 lanes owns slot s: it finds the slot's exact box (a child's from `boxes`, a leaf's from
// its triangles), the 8 boxes are united by three xor-shuffle steps (refit_min / refit_max do not depend on the order: every lane ends with the same
// bits), every lane quantises its own slot.  The record is assembled in LDS — the old record first, so that the bytes of empty slots and the fields
// that stay need no special case — and goes back with five 16-byte stores.  REF_BOXES: a reference's box is ref_boxes' (a tree with split triangles,
// presplit.hpp), not its whole triangle's; without it the kernel is what it was before there were such trees.
template <bool REF_BOXES> __global__ __launch_bounds__(kRefitThreads) void k_refit_nodes(uint4 *nodes, float4 *boxes, const int32_t *level, int n_level, const int32_t *tri_indices, const float4 *triangles,
                                                                                        int tri_float4, const float4 *ref_boxes)
{
	__shared__ uint4 s_node[kNodesPerGroup][kNodeUint4];
	const int g = threadIdx.x / kLanesPerNode, s = threadIdx.x % kLanesPerNode;
	const int k = blockIdx.x * kNodesPerGroup + g;
	const bool valid = k < n_level;
	const size_t node = valid ? (size_t)level[k] : 0;
	if(valid && s < kNodeUint4) s_node[g][s] = nodes[node * kNodeUint4 + s];
	__syncthreads();
	uint8_t *bytes = (uint8_t *)s_node[g];
	RefitBox mine = refit_empty_box();
	uint32_t meta = 0, old_word3 = 0;
	if(valid)
	{
		meta = bytes[kNodeMeta + s];
		old_word3 = s_node[g][0].w;
		const uint32_t child_base = s_node[g][1].x, tri_base = s_node[g][1].y;
		const int kind = refit_slot_kind(meta);
		if(kind == kSlotInternal)
		{
			const size_t child = (size_t)child_base + refit_child_offset(meta);
			const float4 lo = boxes[child * 2], hi = boxes[child * 2 + 1];
			mine = RefitBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
		}
		else if(kind == kSlotLeaf)
		{
			const int count = refit_leaf_count(meta);
			for(int r = 0; r < count; ++r)
			{
				if(REF_BOXES)
				{
					const size_t at = (size_t)tri_base + refit_leaf_offset(meta) + (size_t)r;
					const float4 lo = ref_boxes[at * 2], hi = ref_boxes[at * 2 + 1];
					mine = refit_union(mine, RefitBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}});
					continue;
				}
				const float4 *rec = triangles + (size_t)tri_indices[(size_t)tri_base + refit_leaf_offset(meta) + (size_t)r] * (size_t)tri_float4;
				float p[9];
				load_positions(rec, p);
				mine = refit_union(mine, refit_triangle_box(p));
			}
		}
	}
	RefitBox box = mine;
	int occupied = meta != 0 ? 1 : 0;
	for(int m = 1; m < kLanesPerNode; m <<= 1)
	{
		for(int a = 0; a < 3; ++a)
		{
			box.lo[a] = refit_min(box.lo[a], __shfl_xor(box.lo[a], m));
			box.hi[a] = refit_max(box.hi[a], __shfl_xor(box.hi[a], m));
		}
		occupied |= __shfl_xor(occupied, m);
	}
	if(valid && s == 0)
	{
		boxes[node * 2] = make_float4(box.lo[0], box.lo[1], box.lo[2], 0.0f);
		boxes[node * 2 + 1] = make_float4(box.hi[0], box.hi[1], box.hi[2], 0.0f);
	}
	const bool rewrite = valid && occupied; // (a node without an occupied slot stays as it is: refit.hpp)
	if(rewrite)
	{
		float p[3];
		uint32_t e[3], word3;
		refit_header(box, old_word3, p, &word3, e);
		if(meta != 0)
		{
			uint8_t q[6];
			refit_slot_bytes(box, e, mine, q);
			for(int a = 0; a < 6; ++a) bytes[kNodeQuant + a * 8 + s] = q[a];
		}
		if(s == 0) s_node[g][0] = make_uint4(refit_bits(p[0]), refit_bits(p[1]), refit_bits(p[2]), word3);
	}
	__syncthreads();
	if(rewrite && s < kNodeUint4) nodes[node * kNodeUint4 + s] = s_node[g][s];
}


// The two sums of tree_cost.hpp over nodes [0, n_nodes), n_nodes >= 1.  The lanes of a node read its 80 bytes as five 16-byte loads — a wave reads 640
// contiguous bytes — into LDS, and lane s takes slot s from there.  Node 0, whose union is the root area of every slot, is read at a uniform address
// by every wave and decoded in registers.  The sums are added up across the wave by xor-shuffles, across the workgroup's waves in LDS, and one
// workgroup adds each sum to words[0] (inner_q) and words[1] (leaf_q) with one 64-bit atomic; words[2] takes the flags.  Nobody waits for anybody.
enum CostFlag : uint32_t { kCostFlagRoot = 1u, kCostFlagRatio = 2u };
constexpr int kCostWaves = kRefitThreads / 64;
__global__ __launch_bounds__(kRefitThreads) void k_tree_cost(const uint4 *__restrict__ nodes, int n_nodes, unsigned long long *words)
{
	__shared__ uint4 s_node[kNodesPerGroup][kNodeUint4];
	__shared__ unsigned long long s_sum[kCostWaves][2];
	const int g = threadIdx.x / kLanesPerNode, s = threadIdx.x % kLanesPerNode;
	const int64_t k = (int64_t)blockIdx.x * kNodesPerGroup + g;
	const bool valid = k < (int64_t)n_nodes;
	if(valid && s < kNodeUint4) s_node[g][s] = nodes[(size_t)k * kNodeUint4 + s];
	uint32_t root[kNodeBytes / 4];
	for(int j = 0; j < kNodeUint4; ++j)
	{
		const uint4 v = nodes[j];
		root[j * 4] = v.x; root[j * 4 + 1] = v.y; root[j * 4 + 2] = v.z; root[j * 4 + 3] = v.w;
	}
	const float A = cost_root_area(root);
	__syncthreads();
	uint64_t inner_q = 0, leaf_q = 0;
	if(!cost_root_valid(A))
	{
		if(blockIdx.x == 0 && threadIdx.x == 0) atomicOr(words + 2, (unsigned long long)kCostFlagRoot);
	}
	else if(valid)
	{
		const uint8_t *bytes = (const uint8_t *)s_node[g];
		const uint32_t meta = bytes[kNodeMeta + s];
		if(meta != 0)
		{
			uint32_t q[6], e[3];
			cost_slot_bytes(bytes, s, q, e);
			const CostShare share = cost_slot(meta, cost_area(q, e), A);
			inner_q = share.inner_q;
			leaf_q = share.leaf_q;
			if(!share.ok) atomicOr(words + 2, (unsigned long long)kCostFlagRatio);
		}
	}
	for(int m = 1; m < 64; m <<= 1)
	{
		inner_q += (uint64_t)__shfl_xor((unsigned long long)inner_q, m);
		leaf_q += (uint64_t)__shfl_xor((unsigned long long)leaf_q, m);
	}
	if(threadIdx.x % 64 == 0) { s_sum[threadIdx.x / 64][0] = inner_q; s_sum[threadIdx.x / 64][1] = leaf_q; }
	__syncthreads();
	if(threadIdx.x < 2)
	{
		unsigned long long sum = 0;
		for(int w = 0; w < kCostWaves; ++w) sum += s_sum[w][threadIdx.x];
		if(sum) atomicAdd(words + threadIdx.x, sum);
	}
}

constexpr int kTimingEvents = 4; // start, scatter, references + Woop, nodes

// Everything the refit keeps per context; parked in the context (ctx_attachment), freed by adypt_destroy (the context's device is current then).
struct Refitter {
	TreeLevels tree;           // of the context's tree as it is now: planned at the first update, or handed over by a rebuild
	bool have_plan = false;
	Buffer<float> d_stage;     // the caller's positions and normals on their way to the records: up to 72 B per updated triangle
	StageTimer<kTimingEvents> timer;
	// the cost of the tree (tree_cost.hpp)
	Buffer<unsigned long long> d_cost;  // inner_q, leaf_q, the flags
	StageTimer<2> cost_timer;
	adypt_tree_cost built{};            // the sums of the tree as uploaded or as last rebuilt, once measured (priced anew by every call)
	bool have_built = false;
};

// the levels from one copy of the node array, the lists and the box array on the device (the context is drained)
int ensure_plan(adypt_ctx *c, Refitter *rf, const CtxScene &sc, hipStream_t stream)
{
	if(rf->have_plan) return ADYPT_OK;
	std::vector<uint8_t> nodes((size_t)sc.n_nodes * kNodeBytes);
	CTX_TRY(c, hipMemcpyAsync(nodes.data(), sc.nodes, nodes.size(), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	RefitPlan plan;
	std::string why;
	if(!plan_refit(nodes.data(), sc.n_nodes, sc.n_refs, &plan, &why)) return ctx_fail(c, ADYPT_E_INVALID, "adypt_update_triangles: the node array is not one tree: " + why);
	rf->tree.level_begin = std::move(plan.level_begin);
	CTX_TRY(c, rf->tree.order.alloc(plan.order.size() * sizeof(int32_t)));
	CTX_TRY(c, rf->tree.boxes.alloc((size_t)sc.n_nodes * 2 * sizeof(float4)));
	CTX_TRY(c, hipMemcpyAsync(rf->tree.order, plan.order.data(), plan.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	rf->have_plan = true;
	return ADYPT_OK;
}

// the cost of the context's tree as it is now, on the stream (the context is drained); *ms: the HIP-event time of the kernel
int measure_cost(adypt_ctx *c, Refitter *rf, hipStream_t stream, const adypt_bvh_params &cfg, const char *who, adypt_tree_cost *out, float *ms)
{
	const CtxScene sc = ctx_scene(c);
	if(sc.n_nodes <= 0) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": the tree has no nodes");
	if(sc.n_nodes > kCostMaxNodes) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": more than 2^26 nodes");
	CTX_TRY(c, at_least(rf->d_cost, 3));
	unsigned long long words[3] = {0, 0, 0};
	CTX_TRY(c, hipMemsetAsync(rf->d_cost.get(), 0, sizeof(words), stream));
	CTX_TRY(c, rf->cost_timer.mark(0, stream));
	hipLaunchKernelGGL(k_tree_cost, dim3(grid_of(sc.n_nodes, kNodesPerGroup)), dim3(kRefitThreads), 0, stream, (const uint4 *)sc.nodes, (int)sc.n_nodes, rf->d_cost.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, rf->cost_timer.mark(1, stream));
	CTX_TRY(c, hipMemcpyAsync(words, rf->d_cost.get(), sizeof(words), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	if(words[2] & kCostFlagRoot) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": the root's box has no positive finite area");
	if(words[2] & kCostFlagRatio) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": a slot is not below four times the root's area");
	if(ms) rf->cost_timer.read(ms, 1, 1, false);
	*out = adypt_tree_cost{cost_value((double)cfg.node_sah, (double)cfg.triangle_sah, words[0], words[1]), words[0], words[1], sc.n_nodes};
	return ADYPT_OK;
}

// the reference of the pose policy: measured now unless it has been since the upload or the last rebuild; priced with this call's costs
int built_cost(adypt_ctx *c, Refitter *rf, hipStream_t stream, const adypt_bvh_params &cfg, const char *who, adypt_tree_cost *out)
{
	if(!rf->have_built)
	{
		CTX_STEP(measure_cost(c, rf, stream, cfg, who, &rf->built, nullptr));
		rf->have_built = true;
	}
	*out = rf->built;
	out->cost = cost_value((double)cfg.node_sah, (double)cfg.triangle_sah, out->inner_q, out->leaf_q);
	return ADYPT_OK;
}

}  // namespace

namespace adypt {

hipError_t refit_launch_woop(hipStream_t stream, const float4 *triangles, int tri_float4, const int32_t *tri_indices, int64_t n_refs, float4 *woop)
{
	if(n_refs <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_refit_woop, dim3(grid_of(n_refs, kRefitThreads)), dim3(kRefitThreads), 0, stream, triangles, tri_float4, tri_indices, n_refs, woop);
	return hipGetLastError();
}

hipError_t refit_launch_levels(hipStream_t stream, const TreeLevels &tree, uint4 *nodes, const int32_t *tri_indices, const float4 *triangles, int tri_float4, const float4 *ref_boxes)
{
	for(int l = tree.levels() - 1; l >= 0; --l)
	{
		const int64_t begin = tree.level_begin[(size_t)l], n = tree.level_begin[(size_t)l + 1] - begin;
		if(n <= 0) continue;
		if(ref_boxes) hipLaunchKernelGGL(k_refit_nodes<true>, dim3(grid_of(n, kNodesPerGroup)), dim3(kRefitThreads), 0, stream, nodes, tree.boxes.get(), (const int32_t *)tree.order + begin, (int)n, tri_indices, triangles, tri_float4, ref_boxes);
		else hipLaunchKernelGGL(k_refit_nodes<false>, dim3(grid_of(n, kNodesPerGroup)), dim3(kRefitThreads), 0, stream, nodes, tree.boxes.get(), (const int32_t *)tree.order + begin, (int)n, tri_indices, triangles, tri_float4, ref_boxes);
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess) return e;
	}
	return hipSuccess;
}

void refit_adopt_tree(adypt_ctx *c, TreeLevels &&tree)
{
	Refitter *rf = ctx_state<Refitter>(c, kAttachRefit);
	rf->tree = std::move(tree); // (the old tree's lists and boxes go with `tree`)
	rf->have_plan = true;
	rf->timer.invalidate();
	rf->have_built = false; // (a new tree: its cost is measured when it is first asked for)
}

int refit_begin(adypt_ctx *c)
{
	const CtxScene sc = ctx_scene(c);
	CTX_STEP(ctx_drain(c));
	const CtxInfo i = ctx_info(c);
	Refitter *rf = ctx_state<Refitter>(c, kAttachRefit);
	CTX_STEP(ensure_plan(c, rf, sc, i.stream));
	rf->timer.invalidate();
	CTX_TRY(c, rf->timer.mark(0, i.stream));
	return ADYPT_OK;
}

int refit_tail(adypt_ctx *c)
{
	const CtxScene sc = ctx_scene(c);
	const CtxInfo i = ctx_info(c);
	Refitter *rf = ctx_state<Refitter>(c, kAttachRefit);
	rf->tree.ref_boxes.release(); // (a split tree's clipped boxes were the old pose's: from here on its leaves bound whole triangles, as an SBVH tree's do)
	CTX_TRY(c, rf->timer.mark(1, i.stream));
	CTX_STEP(ctx_expand_references(c));
	CTX_TRY(c, refit_launch_woop(i.stream, (const float4 *)sc.triangles, sc.tri_float4, sc.tri_indices, sc.n_refs, sc.woop));
	CTX_TRY(c, rf->timer.mark(2, i.stream));
	CTX_TRY(c, refit_launch_levels(i.stream, rf->tree, sc.nodes, sc.tri_indices, (const float4 *)sc.triangles, sc.tri_float4));
	CTX_STEP(ctx_refresh_root_card(c)); // (node 0 has new boxes: k_path's root card follows, on the same stream)
	CTX_TRY(c, rf->timer.mark(3, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	rf->timer.complete();
	return adypt_reset(c); // the image, the frozen blocks, the frames parked ahead and the primary-hit cache were the old pose's
}

const char *refit_policy_refused(const adypt_bvh_params *params, const adypt_pose_policy *policy, BuildRequest *request)
{
	const adypt_pose_policy p = *policy;
	*request = BuildRequest{build_cfg(params), p.method, p.radius, p.split_budget};
	if(const char *why = sah_refused(request->cfg)) return why;
	if(!(p.rebuild_above >= 0.0 && std::isfinite(p.rebuild_above))) return "rebuild_above must be a finite number >= 0";
	return method_refused(p.method, p.radius, p.split_budget);
}

int refit_under_policy(adypt_ctx *c, const char *who, const BuildRequest &request, double rebuild_above, adypt_pose_outcome *outcome, const std::function<int()> &refit)
{
	const adypt_bvh_params &cfg = request.cfg;
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	Refitter *rf = ctx_state<Refitter>(c, kAttachRefit);
	adypt_pose_outcome o{};
	CTX_STEP(built_cost(c, rf, i.stream, cfg, who, &o.built)); // (of the tree as it is before this call's refit)
	CTX_STEP(refit());
	const int measured = measure_cost(c, rf, i.stream, cfg, who, &o.refitted, &o.cost_ms);
	if(measured != ADYPT_OK) return ctx_fail(c, measured, std::string(adypt_last_error(c)) + " (the triangles have been updated and the tree refitted; nothing was rebuilt)");
	o.now = o.refitted;
	if(o.refitted.cost > rebuild_above * o.built.cost)
	{
		// (a rebuild that fails has left the refitted tree in place and set the error, under the name of the public rebuild of this shape)
		CTX_STEP(rebuild_own_triangles(c, request, rebuild_entry(request), &o.rebuild));
		o.rebuilt = 1;
		CTX_STEP(built_cost(c, rf, i.stream, cfg, who, &o.now)); // (the rebuild has marked it stale: the new tree's, which is the reference from here on)
	}
	if(outcome) *outcome = o;
	return ADYPT_OK;
}

int multi_each_outcome(adypt_multi *m, const char *who, adypt_pose_outcome *outcome, const std::function<int(adypt_ctx *, adypt_pose_outcome *)> &f)
{
	adypt_pose_outcome head{};
	int k = 0;
	const int r = multi_each(m, [&](adypt_ctx *c) {
		adypt_pose_outcome o{};
		CTX_STEP(f(c, &o));
		if(k++ == 0) head = o;
		else if(o.rebuilt != head.rebuilt || o.refitted.inner_q != head.refitted.inner_q || o.refitted.leaf_q != head.refitted.leaf_q || o.now.inner_q != head.now.inner_q || o.now.leaf_q != head.now.leaf_q ||
		        o.built.inner_q != head.built.inner_q || o.built.leaf_q != head.built.leaf_q)
			return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": device " + std::to_string(k - 1) + " measured or decided otherwise than device 0: the trees differ from here on");
		return (int)ADYPT_OK;
	});
	if(r == ADYPT_OK && outcome) *outcome = head;
	return r;
}

}  // namespace adypt

extern "C" {

int adypt_update_triangles(adypt_ctx *c, int64_t first, int64_t count, const float *positions, const float *normals)
{
	if(!c) return ADYPT_E_INVALID;
	const CtxScene sc = ctx_scene(c);
	if(!positions) return ctx_fail(c, ADYPT_E_INVALID, "adypt_update_triangles: positions is null");
	if(first < 0 || count < 0 || first > sc.n_tris || count > sc.n_tris - first)
		return ctx_fail(c, ADYPT_E_INVALID, "adypt_update_triangles: triangles [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) + ") are not all of the scene's " + std::to_string(sc.n_tris));
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	Refitter *rf = ctx_state<Refitter>(c, kAttachRefit);
	const size_t n_stage = (size_t)count * 9;
	CTX_TRY(c, at_least(rf->d_stage, n_stage * (normals ? 2 : 1)));
	CTX_STEP(refit_begin(c));
	if(count > 0)
	{
		float *d_pos = rf->d_stage, *d_nrm = normals ? d_pos + n_stage : nullptr;
		CTX_TRY(c, hipMemcpyAsync(d_pos, positions, n_stage * sizeof(float), hipMemcpyHostToDevice, i.stream));
		if(normals) CTX_TRY(c, hipMemcpyAsync(d_nrm, normals, n_stage * sizeof(float), hipMemcpyHostToDevice, i.stream));
		hipLaunchKernelGGL(k_refit_scatter, dim3(grid_of(count, kRefitThreads)), dim3(kRefitThreads), 0, i.stream, sc.triangles, sc.tri_float4, first, count, (const float *)d_pos, (const float *)d_nrm);
		CTX_TRY(c, hipGetLastError());
	}
	return refit_tail(c);
}

int adypt_get_tree_cost(adypt_ctx *c, const adypt_bvh_params *params, adypt_tree_cost *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, "adypt_get_tree_cost: out is null");
	const adypt_bvh_params cfg = build_cfg(params);
	if(const char *why = sah_refused(cfg)) return ctx_fail(c, ADYPT_E_INVALID, std::string("adypt_get_tree_cost: ") + why);
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	Refitter *rf = ctx_state<Refitter>(c, kAttachRefit);
	adypt_tree_cost now;
	CTX_STEP(measure_cost(c, rf, i.stream, cfg, "adypt_get_tree_cost", &now, nullptr));
	if(!rf->have_built) { rf->built = now; rf->have_built = true; }
	*out = now;
	return ADYPT_OK;
}

int adypt_update_triangles_auto(adypt_ctx *c, int64_t first, int64_t count, const float *positions, const float *normals, const adypt_bvh_params *params,
                                const adypt_pose_policy *policy, adypt_pose_outcome *outcome)
{
	if(!c) return ADYPT_E_INVALID;
	const char *who = "adypt_update_triangles_auto";
	const CtxScene sc = ctx_scene(c);
	if(!positions) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": positions is null");
	if(!policy) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": policy is null");
	if(first < 0 || count < 0 || first > sc.n_tris || count > sc.n_tris - first)
		return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": triangles [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) + ") are not all of the scene's " + std::to_string(sc.n_tris));
	BuildRequest request;
	if(const char *why = refit_policy_refused(params, policy, &request)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": " + why);
	return refit_under_policy(c, who, request, policy->rebuild_above, outcome, [=]() { return adypt_update_triangles(c, first, count, positions, normals); });
}

int adypt_read_bvh(adypt_ctx *c, void *nodes_out, float *woop_out)
{
	if(!c) return ADYPT_E_INVALID;
	const CtxScene sc = ctx_scene(c);
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	if(nodes_out) CTX_TRY(c, hipMemcpy(nodes_out, sc.nodes, (size_t)sc.n_nodes * kNodeBytes, hipMemcpyDeviceToHost));
	if(woop_out && sc.n_refs > 0) CTX_TRY(c, hipMemcpy(woop_out, sc.woop, (size_t)sc.n_refs * 12 * sizeof(float), hipMemcpyDeviceToHost));
	return ADYPT_OK;
}

int64_t adypt_read_ref_boxes(adypt_ctx *c, float *out)
{
	if(!c) return ADYPT_E_INVALID;
	const CtxScene sc = ctx_scene(c);
	const CtxInfo i = ctx_info(c);
	const Refitter *rf = ctx_state_if_any<Refitter>(c, kAttachRefit);
	if(!rf || !rf->tree.ref_boxes.get() || sc.n_refs <= 0) return 0;
	if(!out) return sc.n_refs;
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	std::vector<float4> boxes((size_t)sc.n_refs * 2);
	CTX_TRY(c, hipMemcpy(boxes.data(), rf->tree.ref_boxes.get(), boxes.size() * sizeof(float4), hipMemcpyDeviceToHost));
	for(int64_t r = 0; r < sc.n_refs; ++r)
	{
		const float4 lo = boxes[(size_t)r * 2], hi = boxes[(size_t)r * 2 + 1];
		float *o = out + r * 6;
		o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = hi.x; o[4] = hi.y; o[5] = hi.z;
	}
	return sc.n_refs;
}

int adypt_get_refit_timing(adypt_ctx *c, float *ms, int capacity)
{
	if(!c || !ms || capacity < 0) return ADYPT_E_INVALID;
	const Refitter *rf = ctx_state_if_any<Refitter>(c, kAttachRefit);
	if(!rf || !rf->timer.completed()) return ctx_fail(c, ADYPT_E_STATE, "adypt_get_refit_timing: nothing has been refitted yet (adypt_update_triangles)");
	return rf->timer.read(ms, capacity, kTimingEvents - 1, true);
}

// the scene is replicated: the same update on every device
int adypt_multi_update_triangles(adypt_multi *m, int64_t first, int64_t count, const float *positions, const float *normals)
{
	// (a bad range is refused by the first context: none has changed)
	return multi_each(m, [=](adypt_ctx *c) { return adypt_update_triangles(c, first, count, positions, normals); });
}

// every device measures its own copy: the sums are integers, so all must agree
int adypt_multi_get_tree_cost(adypt_multi *m, const adypt_bvh_params *params, adypt_tree_cost *out)
{
	adypt_tree_cost head{};
	int k = 0;
	if(m && !out) { multi_set_error(m, "adypt_multi_get_tree_cost: out is null"); return ADYPT_E_INVALID; }
	const int r = multi_each(m, [&](adypt_ctx *c) {
		adypt_tree_cost t{};
		CTX_STEP(adypt_get_tree_cost(c, params, &t));
		if(k++ == 0) head = t;
		else if(t.inner_q != head.inner_q || t.leaf_q != head.leaf_q || t.n_nodes != head.n_nodes)
			return ctx_fail(c, ADYPT_E_HIP, "adypt_multi_get_tree_cost: device " + std::to_string(k - 1) + " holds another tree than device 0");
		return (int)ADYPT_OK;
	});
	if(r == ADYPT_OK) *out = head;
	return r;
}

int adypt_multi_update_triangles_auto(adypt_multi *m, int64_t first, int64_t count, const float *positions, const float *normals, const adypt_bvh_params *params,
                                      const adypt_pose_policy *policy, adypt_pose_outcome *outcome)
{
	// (bad arguments are refused by the first context: none has changed)
	return multi_each_outcome(m, "adypt_multi_update_triangles_auto", outcome,
	                          [=](adypt_ctx *c, adypt_pose_outcome *o) { return adypt_update_triangles_auto(c, first, count, positions, normals, params, policy, o); });
}

}  // extern "C"
