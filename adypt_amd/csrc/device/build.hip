// Rebuilding the tree on the device (include/adypt_hip.h adypt_rebuild_bvh ...; the definition: lbvh.hpp, the cut: wide_cut.hpp, the boxes: refit.hpp).  A
// translation unit of its own: nothing here is part of the tracer's code object.  What one rebuild runs, all on the context's stream after the context
// has been drained, from the triangle records as they are in HBM:
//     k_centroid_box    twice: one partial box per workgroup (xor-shuffles inside a wave, LDS across the waves), then the partials — min / max that do
//                       not depend on the order
//     k_keys            one thread per triangle
//     rocprim::radix_sort_keys on the 62 key bits in use
//     k_radix_tree      one thread per inner node: its children, and their parent links
//     k_bottom_up       one thread per leaf walks towards the root: exact boxes, triangle counts, the DP rows and wide_below.  At an inner node the first
//                       of the two arrivers stops, the second goes on (one atomicAdd on the node's counter between two fences); nobody waits
//     k_emit            one launch per level of the wide tree, the root's first: a thread writes one node's topology and its leaf references and appends
//                       the node's inner children, with the runs that are theirs, to the next level.  Only the queue slot comes from an atomic; where a
//                       node and its references go was decided by the counts.  The host reads the next level's size (4 bytes) between launches
//     (refit.hip)       k_refit_woop, then k_refit_nodes level by level, deepest first, over the queues of k_emit
// adypt_rebuild_bvh_ploc (the definition: ploc.hpp) keeps the keys, the sort and everything from k_emit on, and builds the binary tree bottom up instead:
//     k_ploc_leaves     one thread per leaf: what k_bottom_up writes for a leaf, and the first cluster list
//     per round         k_ploc_nearest (every cluster's choice among the 2 r around it, their boxes staged in LDS), k_ploc_marks (who stays, who
//                       merges), rocprim::exclusive_scan over the marks (new positions and merge ordinals: by position, never by arrival), k_ploc_merge
//                       (the new nodes — k_bottom_up's loop body over children that earlier launches finished — and the next cluster list).  The host
//                       reads the round's two counts (8 bytes) and goes on until one cluster is left; a round without a merge ends the build
//     Stream order is the whole dependency: no atomics on the tree, no fences, nobody waits for another workgroup.
// adypt_rebuild_bvh_ploc_split with a budget above 0 (the definition: presplit.hpp) puts a stage in front of the keys, which counts into "keys":
//     k_centroid_box    twice more, over the triangles' boxes: the scene box, whose area sets the thresholds
//     k_split_hist      twice, one thread per triangle: first the root cells alone (two clips), which bound the level from above, then the walk of the
//                       cells down to that bound (the walk's memory — the waiting halves, the clip's polygons — in LDS, one column per thread).
//                       The cells that split go into a histogram of 24 bins in LDS, then into HBM, by integer atomics; a triangle below the
//                       threshold clips nothing.  The host reads the 24 counts after either (192 bytes) and decides the level
//     k_split_counts    the references of every triangle at that level; rocprim::exclusive_scan over them
//     k_split_emit      ref_tri and ref_box of every reference, at scan + ordinal
//     k_ref_centroid_box, k_ref_keys    the centroid box and the keys over the references
// and from the sort on n is the number of references: the leaves' boxes are ref_box, BinTree::tri() goes through ref_tri, k_emit also records which
// reference went to each position (ref_at), k_gather_ref_boxes puts the boxes into that order, and k_refit_nodes bounds leaf slots by them.  A budget
// of 0, or one under which nothing splits, runs none of this but (in the second case) the scene box and the two k_split_hist.
// Everything is built into new arrays; the context takes them last (ctx_replace_bvh), so a refused or failed call leaves the old tree usable.
#include "ctx_unit.hpp"
#include "refit_internal.hpp"
#include "build_internal.hpp"
#include "lbvh.hpp"
#include "ploc.hpp"
#include "presplit.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <string>
#include <vector>

using namespace adypt;

namespace {

constexpr int kBuildThreads = 256, kEmitThreads = 128;
constexpr int kMaxPartials = 1024;          // workgroups of the first k_centroid_box launch
constexpr int kKeyBits = 62;                // 30 bits of Morton code above 32 bits of index
enum BuildFlag : uint32_t { kFlagCost = 1u, kFlagLayout = 2u };

static_assert(sizeof(CutRow) == 56 && sizeof(WideItem) == 16, "records of the builder");

// the union of a workgroup's boxes -> out[blockIdx.x], 8 floats (lo xyz 0, hi xyz 0): xor-shuffles inside a wave, LDS across the waves
__device__ __forceinline__ void block_union(RefitBox box, float4 *out)
{
	__shared__ float s_box[kBuildThreads / 64][6];
	for(int m = 1; m < 64; m <<= 1)
		for(int k = 0; k < 3; ++k)
		{
			box.lo[k] = refit_min(box.lo[k], __shfl_xor(box.lo[k], m));
			box.hi[k] = refit_max(box.hi[k], __shfl_xor(box.hi[k], m));
		}
	if(threadIdx.x % 64 == 0)
		for(int k = 0; k < 3; ++k) { s_box[threadIdx.x / 64][k] = box.lo[k]; s_box[threadIdx.x / 64][3 + k] = box.hi[k]; }
	__syncthreads();
	if(threadIdx.x != 0) return;
	for(int w = 1; w < kBuildThreads / 64; ++w)
		for(int k = 0; k < 3; ++k) { box.lo[k] = refit_min(box.lo[k], s_box[w][k]); box.hi[k] = refit_max(box.hi[k], s_box[w][3 + k]); }
	out[(size_t)blockIdx.x * 2] = make_float4(box.lo[0], box.lo[1], box.lo[2], 0.0f);
	out[(size_t)blockIdx.x * 2 + 1] = make_float4(box.hi[0], box.hi[1], box.hi[2], 0.0f);
}

enum BoxOf { kOfBoxes = 0, kOfCentroids = 1, kOfTriangles = 2 };
// in: triangle records (kOfCentroids: the box of their centroids; kOfTriangles: of the triangles themselves) or boxes of 8 floats; out[blockIdx.x]: the union
template <int OF> __global__ __launch_bounds__(kBuildThreads) void k_centroid_box(const float4 *in, int tri_float4, int64_t n, float4 *out)
{
	RefitBox box = refit_empty_box();
	for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
	{
		if(OF != kOfBoxes)
		{
			const float4 *rec = in + (size_t)i * (size_t)tri_float4;
			float p[9];
			load_positions(rec, p);
			if(OF == kOfTriangles) box = refit_union(box, refit_triangle_box(p));
			else
				for(int k = 0; k < 3; ++k) { const float v = lbvh_centroid(p, k); box.lo[k] = refit_min(box.lo[k], v); box.hi[k] = refit_max(box.hi[k], v); }
		}
		else
		{
			const float4 lo = in[i * 2], hi = in[i * 2 + 1];
			box = refit_union(box, RefitBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}});
		}
	}
	block_union(box, out);
}

__global__ __launch_bounds__(kBuildThreads) void k_keys(const float4 *triangles, int tri_float4, int64_t n, const float4 *centroid_box, uint64_t *keys)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const float4 lo = centroid_box[0], hi = centroid_box[1];
	const RefitBox box{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
	const float4 *rec = triangles + (size_t)i * (size_t)tri_float4;
	float p[9];
	load_positions(rec, p);
	keys[i] = lbvh_key(p, box, (uint32_t)i);
}

// The binary tree on the device: 2 n - 1 nodes, ids as in lbvh.hpp.  box: 2 float4 per node, lo.w the bits of the triangle count, hi.w those of the height.
struct BinTree {
	int64_t n;
	const uint64_t *keys;
	const int32_t *ref_tri;             // nullptr: one reference per triangle, reference r is triangle r; else presplit.hpp's
	int32_t *left_, *right_, *parent;   // left_, right_: n - 1; parent: 2 n - 1, the root's is -1
	float4 *boxes;
	CutRow *rows;
	uint32_t *wide_below_;
	__device__ __forceinline__ int left(int i) const { return left_[i]; }
	__device__ __forceinline__ int right(int i) const { return right_[i]; }
	__device__ __forceinline__ const CutRow &row(int i) const { return rows[i]; }
	__device__ __forceinline__ uint32_t wide_below(int i) const { return wide_below_[i]; }
	__device__ __forceinline__ bool is_leaf(int i) const { return (int64_t)i >= n - 1; }
	__device__ __forceinline__ int32_t ref(int leaf) const { return (int32_t)(uint32_t)keys[(int64_t)leaf - (n - 1)]; }
	__device__ __forceinline__ int32_t tri(int leaf) const { const int32_t r = ref(leaf); return ref_tri ? ref_tri[r] : r; }
	__device__ __forceinline__ int tri_count(int i) const { return __float_as_int(boxes[(size_t)i * 2].w); }
	__device__ __forceinline__ void box(int i, float lo[3], float hi[3]) const
	{
		const float4 a = boxes[(size_t)i * 2], b = boxes[(size_t)i * 2 + 1];
		lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
	}
};

__global__ __launch_bounds__(kBuildThreads) void k_radix_tree(BinTree t)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= t.n - 1) return;
	int64_t first, last, split;
	lbvh_inner_node(t.keys, t.n, i, &first, &last, &split);
	const int32_t l = lbvh_left_child(t.n, first, split), r = lbvh_right_child(t.n, last, split);
	t.left_[i] = l; t.right_[i] = r;
	t.parent[l] = (int32_t)i; t.parent[r] = (int32_t)i;
}

// arrived: one counter per inner node, zero.  A thread's stores to its node are fenced before it adds to the parent's counter; the thread that finds
// the other one's add there fences again before it reads what lies below (rows of grandchildren too: the fences are cumulative).
__global__ __launch_bounds__(kBuildThreads) void k_bottom_up(BinTree t, const float4 *triangles, int tri_float4, float triangle_sah, float node_sah, uint32_t *arrived, uint32_t *flags)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(j >= t.n) return;
	const int leaf = (int)(t.n - 1 + j);
	{
		const float4 *rec = triangles + (size_t)t.tri(leaf) * (size_t)tri_float4;
		float p[9];
		load_positions(rec, p);
		const RefitBox box = refit_triangle_box(p);
		t.boxes[(size_t)leaf * 2] = make_float4(box.lo[0], box.lo[1], box.lo[2], __int_as_float(1));
		t.boxes[(size_t)leaf * 2 + 1] = make_float4(box.hi[0], box.hi[1], box.hi[2], __int_as_float(0));
		CutRow row;
		cut_leaf_row(cut_area(box.lo, box.hi), triangle_sah, row);
		t.rows[leaf] = row;
		t.wide_below_[leaf] = 0u;
	}
	for(int cur = t.parent[leaf]; cur >= 0; cur = t.parent[cur])
	{
		__threadfence();
		if(atomicAdd(&arrived[cur], 1u) == 0u) return;
		__threadfence();
		const int l = t.left_[cur], r = t.right_[cur];
		const float4 llo = t.boxes[(size_t)l * 2], lhi = t.boxes[(size_t)l * 2 + 1], rlo = t.boxes[(size_t)r * 2], rhi = t.boxes[(size_t)r * 2 + 1];
		const RefitBox box = refit_union(RefitBox{{llo.x, llo.y, llo.z}, {lhi.x, lhi.y, lhi.z}}, RefitBox{{rlo.x, rlo.y, rlo.z}, {rhi.x, rhi.y, rhi.z}});
		const int tc = __float_as_int(rlo.w) + __float_as_int(llo.w), height = 1 + max(__float_as_int(lhi.w), __float_as_int(rhi.w));
		t.boxes[(size_t)cur * 2] = make_float4(box.lo[0], box.lo[1], box.lo[2], __int_as_float(tc));
		t.boxes[(size_t)cur * 2 + 1] = make_float4(box.hi[0], box.hi[1], box.hi[2], __int_as_float(height));
		const CutRow L = t.rows[l], R = t.rows[r];
		CutRow row;
		if(!cut_inner_row(cut_area(box.lo, box.hi), tc, triangle_sah, node_sah, L, R, row)) atomicOr(flags, (uint32_t)kFlagCost);
		t.rows[cur] = row;
		t.wide_below_[cur] = cut_wide_below(t, cur);
	}
}

// ---- PLOC (ploc.hpp).  clusters: node ids in cluster order; nearest: every cluster's choice (-1: none); marks: 1 for a cluster that stays in the list,
// 1 << 32 more for one that merges, and a zero behind the last one — so the exclusive scan's entry [m] holds the round's two counts

// ref_box: the leaves' boxes (2 float4 per reference), or nullptr: the triangles' own
__global__ __launch_bounds__(kBuildThreads) void k_ploc_leaves(BinTree t, const float4 *triangles, int tri_float4, const float4 *ref_box, float triangle_sah, int32_t *clusters, uint32_t *flags)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(j >= t.n) return;
	const int leaf = (int)(t.n - 1 + j);
	RefitBox box;
	if(ref_box)
	{
		const float4 lo = ref_box[(size_t)t.ref(leaf) * 2], hi = ref_box[(size_t)t.ref(leaf) * 2 + 1];
		box = RefitBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
	}
	else
	{
		const float4 *rec = triangles + (size_t)t.tri(leaf) * (size_t)tri_float4;
		float p[9];
		load_positions(rec, p);
		box = refit_triangle_box(p);
	}
	const float area = cut_area(box.lo, box.hi);
	if(!ploc_finite(area)) atomicOr(flags, (uint32_t)kFlagCost);
	t.boxes[(size_t)leaf * 2] = make_float4(box.lo[0], box.lo[1], box.lo[2], __int_as_float(1));
	t.boxes[(size_t)leaf * 2 + 1] = make_float4(box.hi[0], box.hi[1], box.hi[2], __int_as_float(0));
	CutRow row;
	cut_leaf_row(area, triangle_sah, row);
	t.rows[leaf] = row;
	t.wide_below_[leaf] = 0u;
	clusters[j] = leaf;
}

constexpr int kPlocStaged = kBuildThreads + 2 * kPlocMaxRadius;

// the boxes of the positions origin .. origin + kPlocStaged - 1, one array per component: the lanes of a wave read neighbouring positions of one
// component, which are neighbouring banks
struct PlocStaged {
	const float (*s)[kPlocStaged];
	int64_t origin;
	__device__ __forceinline__ RefitBox box(int64_t position) const
	{
		const int k = (int)(position - origin);
		return RefitBox{{s[0][k], s[1][k], s[2][k]}, {s[3][k], s[4][k], s[5][k]}};
	}
};

// One workgroup: the clusters [base, base + 256) and r more on either side, as far as they exist.  Positions outside [0, m) are neither staged nor
// read (ploc_nearest clips its scan to the list), and a position's slot is position - (base - r) < 256 + 2 r <= kPlocStaged.
__global__ __launch_bounds__(kBuildThreads) void k_ploc_nearest(const float4 *boxes, const int32_t *clusters, int64_t m, int r, int32_t *nearest)
{
	__shared__ float s_box[6][kPlocStaged];
	const int64_t base = (int64_t)blockIdx.x * kBuildThreads, origin = base - r;
	for(int k = (int)threadIdx.x; k < kBuildThreads + 2 * r; k += kBuildThreads)
	{
		const int64_t position = origin + k;
		if(position < 0 || position >= m) continue;
		const size_t node = (size_t)clusters[position];
		const float4 lo = boxes[node * 2], hi = boxes[node * 2 + 1];
		s_box[0][k] = lo.x; s_box[1][k] = lo.y; s_box[2][k] = lo.z; s_box[3][k] = hi.x; s_box[4][k] = hi.y; s_box[5][k] = hi.z;
	}
	__syncthreads();
	const int64_t i = base + threadIdx.x;
	if(i >= m) return;
	nearest[i] = (int32_t)ploc_nearest(PlocStaged{s_box, origin}, m, i, r);
}

__global__ __launch_bounds__(kBuildThreads) void k_ploc_marks(const int32_t *nearest, int64_t m, uint64_t *marks)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i > m) return;
	const int role = i < m ? ploc_role(nearest, i) : kPlocLeaves;
	marks[i] = (role != kPlocLeaves ? 1ull : 0ull) | (role == kPlocMerges ? 1ull << 32 : 0ull);
}

// scanned: the exclusive scan of the marks, m + 1 entries.  next: the inner ids from `next` on are given out (ploc.hpp).  A merging cluster writes its
// node as k_bottom_up does, from children that earlier launches finished; every cluster that stays writes its node id to its new position.
__global__ __launch_bounds__(kBuildThreads) void k_ploc_merge(BinTree t, const int32_t *clusters, const int32_t *nearest, const uint64_t *scanned, int64_t m, int64_t next, float triangle_sah, float node_sah,
                                                             int32_t *clusters_out, uint32_t *flags)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= m) return;
	const int role = ploc_role(nearest, i);
	if(role == kPlocLeaves) return;
	const uint64_t mine = scanned[i];
	int32_t cur = clusters[i];
	if(role == kPlocMerges)
	{
		const int l = cur, r = clusters[nearest[i]];
		cur = ploc_merge_id(next, (int64_t)(scanned[m] >> 32), (int64_t)(mine >> 32));
		if(cur < 0 || (int64_t)cur >= t.n - 1) { atomicOr(flags, (uint32_t)kFlagLayout); return; } // (counts that disagree must not turn into a stray store)
		t.left_[cur] = l; t.right_[cur] = r;
		t.parent[l] = cur; t.parent[r] = cur;
		const float4 llo = t.boxes[(size_t)l * 2], lhi = t.boxes[(size_t)l * 2 + 1], rlo = t.boxes[(size_t)r * 2], rhi = t.boxes[(size_t)r * 2 + 1];
		const RefitBox box = refit_union(RefitBox{{llo.x, llo.y, llo.z}, {lhi.x, lhi.y, lhi.z}}, RefitBox{{rlo.x, rlo.y, rlo.z}, {rhi.x, rhi.y, rhi.z}});
		const int tc = __float_as_int(rlo.w) + __float_as_int(llo.w), height = 1 + max(__float_as_int(lhi.w), __float_as_int(rhi.w));
		t.boxes[(size_t)cur * 2] = make_float4(box.lo[0], box.lo[1], box.lo[2], __int_as_float(tc));
		t.boxes[(size_t)cur * 2 + 1] = make_float4(box.hi[0], box.hi[1], box.hi[2], __int_as_float(height));
		const CutRow L = t.rows[l], R = t.rows[r];
		CutRow row;
		if(!cut_inner_row(cut_area(box.lo, box.hi), tc, triangle_sah, node_sah, L, R, row)) atomicOr(flags, (uint32_t)kFlagCost);
		t.rows[cur] = row;
		t.wide_below_[cur] = cut_wide_below(t, cur);
	}
	clusters_out[(uint32_t)mine] = cur;
}

// ref_at[position] = the reference that went there (nothing for nullptr)
struct RefPlaced {
	int32_t *ref_at;
	__device__ __forceinline__ void operator()(const BinTree &t, uint32_t position, int leaf) const { if(ref_at) ref_at[position] = t.ref(leaf); }
};

// items[begin .. begin + count): this level; its inner children are appended from items[begin + count] on, *appended counts them.  n_nodes and n_refs
// bound every store: counts that disagree raise kFlagLayout instead of writing out of range.
__global__ __launch_bounds__(kEmitThreads) void k_emit(BinTree t, WideItem *items, int32_t *order, int64_t begin, int64_t count, uint32_t *appended, int64_t n_nodes, int64_t n_refs, uint4 *nodes,
                                                      int32_t *tri_indices, int32_t *ref_at, uint32_t *flags)
{
	const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(k >= count) return;
	const WideItem it = items[begin + k];
	order[begin + k] = it.w;
	if(it.w < 0 || (int64_t)it.w >= n_nodes) { atomicOr(flags, (uint32_t)kFlagLayout); return; }
	uint32_t rec[20];
	WideItem kids[8];
	const int n_kids = lbvh_emit_node(t, it, rec, tri_indices, (uint32_t)n_refs, kids, RefPlaced{ref_at});
	for(int q = 0; q < kNodeBytes / 16; ++q) nodes[(size_t)it.w * (kNodeBytes / 16) + q] = make_uint4(rec[q * 4], rec[q * 4 + 1], rec[q * 4 + 2], rec[q * 4 + 3]);
	for(int q = 0; q < n_kids; ++q)
	{
		const int64_t at = begin + count + (int64_t)atomicAdd(appended, 1u);
		if(at < n_nodes) items[at] = kids[q];
		else atomicOr(flags, (uint32_t)kFlagLayout);
	}
}

// ---- splitting large triangles (presplit.hpp)

constexpr int kSplitThreads = 64;                                                 // one wave: the walk's memory is 360 B of LDS per thread
constexpr int kSplitWorkWords = kSplitMaxDepth * 6 + 2 * kSplitPolygon * 3;      // the waiting halves, the clip's two polygons
constexpr int kSplitHistWords = kSplitLevels + 1;                                 // the bins, and the number of triangles split

// word w of thread t lies at s[w * kSplitThreads + t]: the lanes of a wave touch neighbouring banks whatever word each of them is at
struct SplitWork {
	float *s; // the thread's column
	__device__ __forceinline__ void put(int depth, const RefitBox &b)
	{
		for(int k = 0; k < 3; ++k) { s[((depth - 1) * 6 + k) * kSplitThreads] = b.lo[k]; s[((depth - 1) * 6 + 3 + k) * kSplitThreads] = b.hi[k]; }
	}
	__device__ __forceinline__ RefitBox get(int depth) const
	{
		RefitBox b;
		for(int k = 0; k < 3; ++k) { b.lo[k] = s[((depth - 1) * 6 + k) * kSplitThreads]; b.hi[k] = s[((depth - 1) * 6 + 3 + k) * kSplitThreads]; }
		return b;
	}
	__device__ __forceinline__ float &v(int polygon, int vertex, int axis) { return s[(kSplitMaxDepth * 6 + (polygon * kSplitPolygon + vertex) * 3 + axis) * kSplitThreads]; }
};

struct SplitBins {
	float s;
	uint32_t *bins; // LDS
	__device__ __forceinline__ void split(float area) { atomicAdd(&bins[presplit_bin(area, s)], 1u); }
	__device__ __forceinline__ void leaf(const RefitBox &, int) {}
};
struct SplitNothing {
	__device__ __forceinline__ void split(float) {}
	__device__ __forceinline__ void leaf(const RefitBox &, int) {}
};
// a triangle's references go to ref_tri / ref_box [base, base + its count); limit bounds every store
struct SplitLeaves {
	int32_t tri, *ref_tri;
	float4 *ref_box;
	int64_t base, limit;
	__device__ __forceinline__ void split(float) {}
	__device__ __forceinline__ void leaf(const RefitBox &b, int ordinal)
	{
		const int64_t r = base + ordinal;
		if(r >= limit) return;
		ref_tri[r] = tri;
		ref_box[r * 2] = make_float4(b.lo[0], b.lo[1], b.lo[2], __int_as_float(1));
		ref_box[r * 2 + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f);
	}
};

__device__ __forceinline__ float scene_area(const float4 *scene_box)
{
	const float4 lo = scene_box[0], hi = scene_box[1];
	const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
	return cut_area(l, h);
}

// Tried and dropped: running the three walks over a compacted list of the triangles whose root cell is above the bound's threshold (one more kernel and 4 B
// per triangle).  Bench scene, the stage as a whole: 3.86 -> 3.77 ms at budget 0.1, 3.68 -> 3.14 ms at 0.3 — the time is in the walks themselves
// (1.2 - 1.3 ms each in a kernel trace; the root pass, two clips for every triangle, 0.06 ms), not in idle lanes.
// hist: kSplitLevels counters, zero.  ROOTS: only the root cells that split are counted (presplit_root_bin); else every cell of the walk down to `level`
template <bool ROOTS> __global__ __launch_bounds__(kSplitThreads) void k_split_hist(const float4 *triangles, int tri_float4, int64_t n, const float4 *scene_box, int level, unsigned long long *hist)
{
	__shared__ float s_work[kSplitWorkWords * kSplitThreads];
	__shared__ uint32_t s_bins[kSplitLevels];
	if(threadIdx.x < kSplitLevels) s_bins[threadIdx.x] = 0u;
	__syncthreads();
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n)
	{
		float p[9];
		load_positions(triangles + (size_t)i * (size_t)tri_float4, p);
		const float s = scene_area(scene_box);
		SplitWork work{s_work + threadIdx.x};
		SplitBins bins{s, s_bins};
		if(ROOTS)
		{
			const int bin = presplit_root_bin(p, s, work);
			if(bin >= 0) atomicAdd(&s_bins[bin], 1u);
		}
		else presplit_walk(p, presplit_threshold(s, level), work, bins);
	}
	__syncthreads();
	if(threadIdx.x < kSplitLevels && s_bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_bins[threadIdx.x]);
}

// counts: n + 1 entries, the last one 0 (so that the exclusive scan's entry [n] is the number of references); *n_split: the triangles with several
__global__ __launch_bounds__(kSplitThreads) void k_split_counts(const float4 *triangles, int tri_float4, int64_t n, const float4 *scene_box, int level, uint32_t *counts, unsigned long long *n_split)
{
	__shared__ float s_work[kSplitWorkWords * kSplitThreads];
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i > n) return;
	uint32_t count = 0;
	if(i < n)
	{
		float p[9];
		load_positions(triangles + (size_t)i * (size_t)tri_float4, p);
		SplitWork work{s_work + threadIdx.x};
		SplitNothing nothing;
		count = (uint32_t)presplit_walk(p, presplit_threshold(scene_area(scene_box), level), work, nothing);
		if(count > 1u) atomicAdd(n_split, 1ull);
	}
	counts[i] = count;
}

// offsets: the exclusive scan of counts, n + 1 entries
__global__ __launch_bounds__(kSplitThreads) void k_split_emit(const float4 *triangles, int tri_float4, int64_t n, const float4 *scene_box, int level, const uint32_t *counts, const uint32_t *offsets, int64_t n_refs,
                                                              int32_t *ref_tri, float4 *ref_box, uint32_t *flags)
{
	__shared__ float s_work[kSplitWorkWords * kSplitThreads];
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	if(i == n - 1 && (int64_t)offsets[n] != n_refs) atomicOr(flags, (uint32_t)kFlagLayout); // (the histogram and the counts disagree)
	const int64_t base = (int64_t)offsets[i];
	float p[9];
	load_positions(triangles + (size_t)i * (size_t)tri_float4, p);
	if(counts[i] == 1u)
	{
		if(base >= n_refs) return;
		const RefitBox b = refit_triangle_box(p);
		ref_tri[base] = (int32_t)i;
		ref_box[base * 2] = make_float4(b.lo[0], b.lo[1], b.lo[2], __int_as_float(0));
		ref_box[base * 2 + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f);
		return;
	}
	SplitWork work{s_work + threadIdx.x};
	SplitLeaves leaves{(int32_t)i, ref_tri, ref_box, base, n_refs};
	presplit_walk(p, presplit_threshold(scene_area(scene_box), level), work, leaves);
}

// the centroid of reference r for its key: ref_box[2 r].w tells whether its triangle is split
__device__ __forceinline__ void ref_centroid(const float4 *triangles, int tri_float4, const int32_t *ref_tri, const float4 *ref_box, int64_t r, float c[3])
{
	const float4 lo = ref_box[r * 2], hi = ref_box[r * 2 + 1];
	if(__float_as_int(lo.w) != 0)
	{
		const RefitBox b{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
		for(int k = 0; k < 3; ++k) c[k] = presplit_centroid(b, k);
		return;
	}
	float p[9];
	load_positions(triangles + (size_t)ref_tri[r] * (size_t)tri_float4, p);
	for(int k = 0; k < 3; ++k) c[k] = lbvh_centroid(p, k);
}

__global__ __launch_bounds__(kBuildThreads) void k_ref_centroid_box(const float4 *triangles, int tri_float4, const int32_t *ref_tri, const float4 *ref_box, int64_t n_refs, float4 *out)
{
	RefitBox box = refit_empty_box();
	for(int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_refs; r += (int64_t)gridDim.x * blockDim.x)
	{
		float c[3];
		ref_centroid(triangles, tri_float4, ref_tri, ref_box, r, c);
		for(int k = 0; k < 3; ++k) { box.lo[k] = refit_min(box.lo[k], c[k]); box.hi[k] = refit_max(box.hi[k], c[k]); }
	}
	block_union(box, out);
}

__global__ __launch_bounds__(kBuildThreads) void k_ref_keys(const float4 *triangles, int tri_float4, const int32_t *ref_tri, const float4 *ref_box, int64_t n_refs, const float4 *centroid_box, uint64_t *keys)
{
	const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(r >= n_refs) return;
	const float4 lo = centroid_box[0], hi = centroid_box[1];
	const RefitBox box{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
	float c[3];
	ref_centroid(triangles, tri_float4, ref_tri, ref_box, r, c);
	keys[r] = lbvh_key_of(c, box, (uint32_t)r);
}

// out[position] = the box of the reference that k_emit put there (ref_at: zero where counts disagreed, so never out of range)
__global__ __launch_bounds__(kBuildThreads) void k_gather_ref_boxes(const int32_t *ref_at, const float4 *ref_box, int64_t n_refs, float4 *out)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n_refs) return;
	const int64_t r = ref_at[i];
	const float4 lo = ref_box[r * 2], hi = ref_box[r * 2 + 1];
	out[i * 2] = make_float4(lo.x, lo.y, lo.z, 0.0f);
	out[i * 2 + 1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
}

constexpr int kTimingEvents = 7; // start, keys, sort, tree, bottom-up, emission, Woop + nodes

// The scratch of a rebuild, kept for the next pose: see adypt_hip.h for the bytes per triangle
struct Builder {
	Buffer<uint64_t> keys, sorted;
	Buffer<uint8_t> sort_tmp;
	Buffer<int32_t> left, right, parent;
	Buffer<float4> boxes, partial;
	Buffer<CutRow> rows;
	Buffer<uint32_t> wide_below, arrived, words; // words: [0] the flags, [1] the next level's count
	Buffer<int32_t> clusters, nearest;           // PLOC: two cluster lists, the choices
	Buffer<uint64_t> marks, scanned;             // PLOC: n + 1 each
	// pre-split (presplit.hpp): 36 B per reference (ref_tri, ref_box) and 4 B more for the emitted order (ref_at); 8 B per triangle (counts, their scan)
	Buffer<int32_t> ref_tri, ref_at;
	Buffer<float4> ref_box;
	Buffer<uint32_t> split_counts, split_offsets;
	Buffer<unsigned long long> hist;             // kSplitHistWords
	int32_t last_presplit[2] = {-1, 0};          // the chosen level, the triangles split
	bool last_ploc = false;
	StageTimer<kTimingEvents> timer;
	adypt_rebuild_info last{};
};

// the PLOC rounds: the tree, boxes, counts, rows and wide_below of every node.  The caller has cleared the flags (b->words).
int ploc_rounds(adypt_ctx *c, Builder *b, hipStream_t stream, const BinTree &t, const float4 *tris, int tri_float4, const float4 *ref_box, const adypt_bvh_params &cfg, int radius, const char *who)
{
	const int64_t n = t.n;
	int32_t *list[2] = {b->clusters.get(), b->clusters.get() + n};
	hipLaunchKernelGGL(k_ploc_leaves, dim3(grid_of(n, kBuildThreads)), dim3(kBuildThreads), 0, stream, t, tris, tri_float4, ref_box, cfg.triangle_sah, list[0], b->words.get());
	CTX_TRY(c, hipGetLastError());
	for(int64_t m = n, next = n - 1; m > 1;)
	{
		hipLaunchKernelGGL(k_ploc_nearest, dim3(grid_of(m, kBuildThreads)), dim3(kBuildThreads), 0, stream, (const float4 *)t.boxes, (const int32_t *)list[0], m, radius, b->nearest.get());
		CTX_TRY(c, hipGetLastError());
		hipLaunchKernelGGL(k_ploc_marks, dim3(grid_of(m + 1, kBuildThreads)), dim3(kBuildThreads), 0, stream, (const int32_t *)b->nearest.get(), m, b->marks.get());
		CTX_TRY(c, hipGetLastError());
		size_t scan_bytes = 0; // (of this round's m + 1 entries: never more than what was allocated for n + 1, and checked, since rocPRIM takes the pointer as it is)
		CTX_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, b->marks.get(), b->scanned.get(), (uint64_t)0, (size_t)(m + 1), rocprim::plus<uint64_t>(), stream));
		if(scan_bytes > b->sort_tmp.bytes()) return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": the scan asks for more temporary storage than it did for the whole list");
		CTX_TRY(c, rocprim::exclusive_scan((void *)b->sort_tmp.get(), scan_bytes, b->marks.get(), b->scanned.get(), (uint64_t)0, (size_t)(m + 1), rocprim::plus<uint64_t>(), stream));
		hipLaunchKernelGGL(k_ploc_merge, dim3(grid_of(m, kBuildThreads)), dim3(kBuildThreads), 0, stream, t, (const int32_t *)list[0], (const int32_t *)b->nearest.get(), (const uint64_t *)b->scanned.get(), m, next,
		                   cfg.triangle_sah, cfg.node_sah, list[1], b->words.get());
		CTX_TRY(c, hipGetLastError());
		uint64_t counts = 0;
		uint32_t flags = 0;
		CTX_TRY(c, hipMemcpyAsync(&counts, b->scanned.get() + m, sizeof(counts), hipMemcpyDeviceToHost, stream));
		CTX_TRY(c, hipMemcpyAsync(&flags, b->words.get(), sizeof(flags), hipMemcpyDeviceToHost, stream));
		CTX_TRY(c, hipStreamSynchronize(stream));
		const int64_t stay = (int64_t)(uint32_t)counts, merges = (int64_t)(counts >> 32);
		if(flags & kFlagCost) return ADYPT_OK; // (the caller reads the flags again and refuses)
		if(flags & kFlagLayout) return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": the merges of a round do not add up to the counted ones");
		if(merges <= 0 || stay != m - merges) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": a round merged nothing (areas that are infinite or NaN)");
		next -= merges;
		m = stay;
		std::swap(list[0], list[1]);
	}
	return ADYPT_OK;
}

// The stage in front of the keys (presplit.hpp): the level for `budget`, and, where that splits anything, ref_tri and ref_box of *n_refs references in
// the builder's scratch.  *n_refs == n: nothing is split and nothing was written.  The caller has cleared the flags (b->words).
int presplit_stage(adypt_ctx *c, Builder *b, hipStream_t stream, const float4 *tris, int tri_float4, int64_t n, double budget, const char *who, int64_t *n_refs, int *level)
{
	*n_refs = n;
	*level = -1;
	size_t scan_bytes = 0;
	CTX_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), stream));
	CTX_TRY(c, at_least(b->partial, (size_t)(kMaxPartials + 2) * 2)); CTX_TRY(c, at_least(b->hist, (size_t)kSplitHistWords));
	CTX_TRY(c, at_least(b->split_counts, (size_t)n + 1)); CTX_TRY(c, at_least(b->split_offsets, (size_t)n + 1)); CTX_TRY(c, at_least(b->sort_tmp, scan_bytes));
	const unsigned n_partial = std::min<unsigned>(grid_of(n, kBuildThreads), kMaxPartials);
	float4 *scene_box = b->partial.get() + (size_t)(kMaxPartials + 1) * 2;
	CTX_TRY(c, hipMemsetAsync(b->hist.get(), 0, kSplitHistWords * sizeof(unsigned long long), stream));
	hipLaunchKernelGGL(k_centroid_box<kOfTriangles>, dim3(n_partial), dim3(kBuildThreads), 0, stream, tris, tri_float4, n, b->partial.get());
	CTX_TRY(c, hipGetLastError());
	hipLaunchKernelGGL(k_centroid_box<kOfBoxes>, dim3(1), dim3(kBuildThreads), 0, stream, (const float4 *)b->partial.get(), 0, (int64_t)n_partial, scene_box);
	CTX_TRY(c, hipGetLastError());
	// the root cells first: no level above the one at which they alone fill the budget can be chosen, so the walk need not go below it (presplit.hpp)
	hipLaunchKernelGGL(k_split_hist<true>, dim3(grid_of(n, kSplitThreads)), dim3(kSplitThreads), 0, stream, tris, tri_float4, n, (const float4 *)scene_box, 0, b->hist.get());
	CTX_TRY(c, hipGetLastError());
	unsigned long long hist[kSplitLevels];
	uint64_t bins[kSplitLevels];
	CTX_TRY(c, hipMemcpyAsync(hist, b->hist.get(), sizeof(hist), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	for(int l = 0; l < kSplitLevels; ++l) bins[l] = hist[l];
	int64_t extra = 0;
	const int64_t allowed = presplit_allowed(budget, n);
	const int top = presplit_level(bins, allowed, &extra);
	if(top < 0) return ADYPT_OK;
	CTX_TRY(c, hipMemsetAsync(b->hist.get(), 0, kSplitLevels * sizeof(unsigned long long), stream));
	hipLaunchKernelGGL(k_split_hist<false>, dim3(grid_of(n, kSplitThreads)), dim3(kSplitThreads), 0, stream, tris, tri_float4, n, (const float4 *)scene_box, top, b->hist.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, hipMemcpyAsync(hist, b->hist.get(), sizeof(hist), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	for(int l = 0; l < kSplitLevels; ++l) bins[l] = hist[l];
	*level = presplit_level(bins, allowed, &extra, top);
	if(extra == 0) return ADYPT_OK;
	if(n + extra > ((int64_t)1 << 30)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": more than 2^30 references");
	const int64_t total = n + extra;
	CTX_TRY(c, at_least(b->ref_tri, (size_t)total)); CTX_TRY(c, at_least(b->ref_box, (size_t)total * 2)); CTX_TRY(c, at_least(b->ref_at, (size_t)total));
	hipLaunchKernelGGL(k_split_counts, dim3(grid_of(n + 1, kSplitThreads)), dim3(kSplitThreads), 0, stream, tris, tri_float4, n, (const float4 *)scene_box, *level, b->split_counts.get(), b->hist.get() + kSplitLevels);
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, rocprim::exclusive_scan((void *)b->sort_tmp.get(), scan_bytes, b->split_counts.get(), b->split_offsets.get(), 0u, (size_t)(n + 1), rocprim::plus<uint32_t>(), stream));
	// (a reference that the counts leave out would be read by the keys: zero is triangle 0 with an empty-ish box, never a stray index)
	CTX_TRY(c, hipMemsetAsync(b->ref_tri.get(), 0, (size_t)total * sizeof(int32_t), stream));
	CTX_TRY(c, hipMemsetAsync(b->ref_box.get(), 0, (size_t)total * 2 * sizeof(float4), stream));
	hipLaunchKernelGGL(k_split_emit, dim3(grid_of(n, kSplitThreads)), dim3(kSplitThreads), 0, stream, tris, tri_float4, n, (const float4 *)scene_box, *level, (const uint32_t *)b->split_counts.get(),
	                   (const uint32_t *)b->split_offsets.get(), total, b->ref_tri.get(), b->ref_box.get(), b->words.get());
	CTX_TRY(c, hipGetLastError());
	*n_refs = total;
	return ADYPT_OK;
}

// The tree `q` names (build_request.hpp, its checks made): the linear one, or PLOC with q.radius, and with triangles split where q.split_budget > 0
// Of the n_tris records at `tris`: the context's own (geometry null), or new ones that the context takes together with their tree
int rebuild(adypt_ctx *c, const BuildRequest &q, const char *who, adypt_rebuild_info *out, const float4 *tris, int64_t n_tris, NewGeometry *geometry = nullptr)
{
	const bool ploc = q.method == kBuildPloc;
	const double budget = q.split_budget;
	const CtxScene sc = ctx_scene(c); // (of it: the layout of a record)
	if(n_tris > ((int64_t)1 << 30)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": more than 2^30 triangles");
	CTX_STEP(ctx_drain(c));
	const hipStream_t stream = ctx_info(c).stream;
	Builder *b = ctx_state<Builder>(c, kAttachBuild);
	int64_t n = n_tris; // the leaves of the binary tree: the references
	int level = -1;
	if(budget > 0.0)
	{
		b->timer.invalidate();
		CTX_TRY(c, at_least(b->words, 2));
		CTX_TRY(c, b->timer.mark(0, stream));
		CTX_TRY(c, hipMemsetAsync(b->words.get(), 0, 2 * sizeof(uint32_t), stream));
		CTX_STEP(presplit_stage(c, b, stream, tris, sc.tri_float4, n_tris, budget, who, &n, &level));
	}
	const bool split = n != n_tris;
	const size_t n_bin = (size_t)(2 * n - 1), n_inner = (size_t)(n - 1);
	size_t sort_bytes = 0;
	CTX_TRY(c, rocprim::radix_sort_keys(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0u, (unsigned)kKeyBits, stream));
	size_t scan_bytes = 0;
	if(ploc) CTX_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), stream));
	if(split && b->sort_tmp.bytes() < std::max(sort_bytes, scan_bytes)) CTX_TRY(c, hipStreamSynchronize(stream)); // (the split stage's scan is using what is about to be given back)
	CTX_TRY(c, at_least(b->keys, (size_t)n)); CTX_TRY(c, at_least(b->sorted, (size_t)n)); CTX_TRY(c, at_least(b->sort_tmp, std::max(sort_bytes, scan_bytes)));
	CTX_TRY(c, at_least(b->left, n_inner)); CTX_TRY(c, at_least(b->right, n_inner)); CTX_TRY(c, at_least(b->parent, n_bin));
	CTX_TRY(c, at_least(b->boxes, n_bin * 2)); CTX_TRY(c, at_least(b->partial, (size_t)(kMaxPartials + 2) * 2));
	CTX_TRY(c, at_least(b->rows, n_bin)); CTX_TRY(c, at_least(b->wide_below, n_bin)); CTX_TRY(c, at_least(b->words, 2));
	if(ploc)
	{
		CTX_TRY(c, at_least(b->clusters, (size_t)n * 2)); CTX_TRY(c, at_least(b->nearest, (size_t)n));
		CTX_TRY(c, at_least(b->marks, (size_t)n + 1)); CTX_TRY(c, at_least(b->scanned, (size_t)n + 1));
	}
	else CTX_TRY(c, at_least(b->arrived, n_inner));
	if(!(budget > 0.0))
	{
		b->timer.invalidate();
		CTX_TRY(c, b->timer.mark(0, stream));
	}
	// ---- keys
	const unsigned n_partial = std::min<unsigned>(grid_of(n, kBuildThreads), kMaxPartials);
	float4 *centroid_box = b->partial.get() + (size_t)kMaxPartials * 2;
	if(split) hipLaunchKernelGGL(k_ref_centroid_box, dim3(n_partial), dim3(kBuildThreads), 0, stream, tris, sc.tri_float4, (const int32_t *)b->ref_tri.get(), (const float4 *)b->ref_box.get(), n, b->partial.get());
	else hipLaunchKernelGGL(k_centroid_box<kOfCentroids>, dim3(n_partial), dim3(kBuildThreads), 0, stream, tris, sc.tri_float4, n, b->partial.get());
	CTX_TRY(c, hipGetLastError());
	hipLaunchKernelGGL(k_centroid_box<kOfBoxes>, dim3(1), dim3(kBuildThreads), 0, stream, (const float4 *)b->partial.get(), 0, (int64_t)n_partial, centroid_box);
	CTX_TRY(c, hipGetLastError());
	if(split) hipLaunchKernelGGL(k_ref_keys, dim3(grid_of(n, kBuildThreads)), dim3(kBuildThreads), 0, stream, tris, sc.tri_float4, (const int32_t *)b->ref_tri.get(), (const float4 *)b->ref_box.get(), n, (const float4 *)centroid_box, b->keys.get());
	else hipLaunchKernelGGL(k_keys, dim3(grid_of(n, kBuildThreads)), dim3(kBuildThreads), 0, stream, tris, sc.tri_float4, n, (const float4 *)centroid_box, b->keys.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, b->timer.mark(1, stream));
	// ---- sort
	CTX_TRY(c, rocprim::radix_sort_keys((void *)b->sort_tmp.get(), sort_bytes, b->keys.get(), b->sorted.get(), (size_t)n, 0u, (unsigned)kKeyBits, stream));
	CTX_TRY(c, b->timer.mark(2, stream));
	BinTree t{n, b->sorted.get(), split ? (const int32_t *)b->ref_tri.get() : nullptr, b->left.get(), b->right.get(), b->parent.get(), b->boxes.get(), b->rows.get(), b->wide_below.get()};
	CTX_TRY(c, hipMemsetAsync(b->parent.get(), 0xff, sizeof(int32_t), stream)); // the root's
	if(!split) CTX_TRY(c, hipMemsetAsync(b->words.get(), 0, 2 * sizeof(uint32_t), stream)); // (the split stage has cleared them, and may have raised one)
	if(ploc)
	{
		// ---- the PLOC tree with its boxes, counts and cut, round by round
		CTX_STEP(ploc_rounds(c, b, stream, t, tris, sc.tri_float4, split ? (const float4 *)b->ref_box.get() : nullptr, q.cfg, q.radius, who));
		CTX_TRY(c, b->timer.mark(3, stream));
	}
	else
	{
		// ---- the radix tree
		if(n_inner)
		{
			hipLaunchKernelGGL(k_radix_tree, dim3(grid_of(n - 1, kBuildThreads)), dim3(kBuildThreads), 0, stream, t);
			CTX_TRY(c, hipGetLastError());
		}
		CTX_TRY(c, b->timer.mark(3, stream));
		// ---- boxes, counts and the cut, bottom up
		CTX_TRY(c, hipMemsetAsync(b->arrived.get(), 0, std::max<size_t>(n_inner, 1) * sizeof(uint32_t), stream));
		hipLaunchKernelGGL(k_bottom_up, dim3(grid_of(n, kBuildThreads)), dim3(kBuildThreads), 0, stream, t, tris, sc.tri_float4, q.cfg.triangle_sah, q.cfg.node_sah, b->arrived.get(), b->words.get());
		CTX_TRY(c, hipGetLastError());
	}
	CTX_TRY(c, b->timer.mark(4, stream));
	uint32_t root_wide = 0, flags = 0;
	float4 root_hi;
	CTX_TRY(c, hipMemcpyAsync(&root_wide, b->wide_below.get(), sizeof(root_wide), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipMemcpyAsync(&root_hi, b->boxes.get() + 1, sizeof(root_hi), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipMemcpyAsync(&flags, b->words.get(), sizeof(flags), hipMemcpyDeviceToHost, stream));
	unsigned long long n_split = 0;
	if(split) CTX_TRY(c, hipMemcpyAsync(&n_split, b->hist.get() + kSplitLevels, sizeof(n_split), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	if(flags & kFlagLayout) return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": the references do not add up to the counted ones");
	if(flags & kFlagCost) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": the SAH costs of this scene are not finite numbers below FLT_MAX (vertices that are NaN, infinite or huge)");
	// ---- the wide tree, top down, into new arrays
	const int64_t n_nodes = std::max<uint32_t>(root_wide, 1u), n_refs = n;
	Buffer<uint4> nodes;
	Buffer<int32_t> tri_indices;
	Buffer<float4> woop;
	TreeLevels tree; // order: the queues of k_emit
	Buffer<WideItem> items;
	CTX_TRY(c, at_least(nodes, (size_t)n_nodes * (kNodeBytes / 16))); CTX_TRY(c, at_least(tri_indices, (size_t)n_refs)); CTX_TRY(c, at_least(woop, (size_t)n_refs * 3));
	CTX_TRY(c, at_least(tree.order, (size_t)n_nodes)); CTX_TRY(c, at_least(tree.boxes, (size_t)n_nodes * 2)); CTX_TRY(c, at_least(items, (size_t)n_nodes));
	CTX_TRY(c, hipMemsetAsync(nodes.get(), 0, (size_t)n_nodes * kNodeBytes, stream));
	CTX_TRY(c, hipMemsetAsync(tri_indices.get(), 0, (size_t)n_refs * sizeof(int32_t), stream));
	if(split)
	{
		CTX_TRY(c, at_least(tree.ref_boxes, (size_t)n_refs * 2));
		CTX_TRY(c, hipMemsetAsync(b->ref_at.get(), 0, (size_t)n_refs * sizeof(int32_t), stream));
	}
	const WideItem root{0, 0, 1u, 0u};
	CTX_TRY(c, hipMemcpyAsync(items.get(), &root, sizeof(root), hipMemcpyHostToDevice, stream));
	tree.level_begin.assign(1, 0);
	for(int64_t begin = 0, count = 1; count > 0;)
	{
		uint32_t *appended = b->words.get() + 1;
		CTX_TRY(c, hipMemsetAsync(appended, 0, sizeof(uint32_t), stream));
		hipLaunchKernelGGL(k_emit, dim3(grid_of(count, kEmitThreads)), dim3(kEmitThreads), 0, stream, t, items.get(), tree.order.get(), begin, count, appended, n_nodes, n_refs, nodes.get(), tri_indices.get(),
		                   split ? b->ref_at.get() : nullptr, b->words.get());
		CTX_TRY(c, hipGetLastError());
		uint32_t words[2] = {0, 0};
		CTX_TRY(c, hipMemcpyAsync(words, b->words.get(), sizeof(words), hipMemcpyDeviceToHost, stream));
		CTX_TRY(c, hipStreamSynchronize(stream));
		begin += count;
		tree.level_begin.push_back(begin);
		count = (int64_t)words[1];
		if((words[0] & kFlagLayout) || begin + count > n_nodes) return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": the emitted nodes do not add up to the counted ones");
	}
	if(tree.level_begin.back() != n_nodes) return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": the emitted nodes do not add up to the counted ones");
	CTX_TRY(c, b->timer.mark(5, stream));
	// ---- Woop data and the node records: the refit's kernels, deepest level first
	CTX_TRY(c, refit_launch_woop(stream, tris, sc.tri_float4, tri_indices.get(), n_refs, woop.get()));
	if(split)
	{
		hipLaunchKernelGGL(k_gather_ref_boxes, dim3(grid_of(n_refs, kBuildThreads)), dim3(kBuildThreads), 0, stream, (const int32_t *)b->ref_at.get(), (const float4 *)b->ref_box.get(), n_refs, tree.ref_boxes.get());
		CTX_TRY(c, hipGetLastError());
	}
	CTX_TRY(c, refit_launch_levels(stream, tree, nodes.get(), tri_indices.get(), tris, sc.tri_float4, split ? (const float4 *)tree.ref_boxes.get() : nullptr));
	CTX_TRY(c, b->timer.mark(6, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	// ---- the context takes the new tree
	if(geometry) CTX_STEP(ctx_replace_geometry(c, geometry, &nodes, &tri_indices, &woop, n_nodes, n_refs));
	else CTX_STEP(ctx_replace_bvh(c, &nodes, &tri_indices, &woop, n_nodes, n_refs));
	b->last = adypt_rebuild_info{n_nodes, n_refs, tree.levels(), __builtin_bit_cast(int32_t, root_hi.w)};
	refit_adopt_tree(c, std::move(tree));
	b->timer.complete();
	b->last_ploc = ploc;
	b->last_presplit[0] = level;
	b->last_presplit[1] = (int32_t)n_split;
	if(out) *out = b->last;
	return ADYPT_OK;
}

}  // namespace

int adypt::rebuild_own_triangles(adypt_ctx *c, const BuildRequest &q, const char *who, adypt_rebuild_info *out)
{
	CTX_TRY(c, hipSetDevice(ctx_info(c).device));
	return rebuild(c, q, who, out, (const float4 *)ctx_scene(c).triangles, ctx_scene(c).n_tris);
}

int adypt::build_for_triangles(adypt_ctx *c, const BuildRequest &q, const char *who, const float4 *triangles, NewGeometry *geometry, adypt_rebuild_info *out)
{
	return rebuild(c, q, who, out, triangles, geometry->n_tris, geometry);
}

// what the three entries below have in common; each applies the part of method_refused that can fail for its shape of request
static int rebuild_entry_point(adypt_ctx *c, const BuildRequest &q, const char *who, adypt_rebuild_info *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(const char *why = request_refused(q)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": " + why);
	return rebuild_own_triangles(c, q, who, out);
}

extern "C" {

int adypt_rebuild_bvh(adypt_ctx *c, const adypt_bvh_params *params, adypt_rebuild_info *out) { return rebuild_entry_point(c, request_linear(params), "adypt_rebuild_bvh", out); }

int adypt_rebuild_bvh_ploc(adypt_ctx *c, const adypt_bvh_params *params, int radius, adypt_rebuild_info *out) { return rebuild_entry_point(c, request_ploc(params, radius), "adypt_rebuild_bvh_ploc", out); }

int adypt_rebuild_bvh_ploc_split(adypt_ctx *c, const adypt_bvh_params *params, int radius, double split_budget, adypt_rebuild_info *out)
{
	return rebuild_entry_point(c, request_ploc(params, radius, split_budget), "adypt_rebuild_bvh_ploc_split", out);
}

int adypt_get_rebuild_presplit(adypt_ctx *c, int32_t out[2])
{
	if(!c || !out) return ADYPT_E_INVALID;
	const Builder *b = ctx_state_if_any<Builder>(c, kAttachBuild);
	if(!b || !b->timer.completed()) return ctx_fail(c, ADYPT_E_STATE, "adypt_get_rebuild_presplit: nothing has been rebuilt yet (adypt_rebuild_bvh)");
	out[0] = b->last_presplit[0]; out[1] = b->last_presplit[1];
	return ADYPT_OK;
}

int adypt_get_rebuild_timing(adypt_ctx *c, float *ms, int capacity)
{
	if(!c || !ms || capacity < 0) return ADYPT_E_INVALID;
	const Builder *b = ctx_state_if_any<Builder>(c, kAttachBuild);
	if(!b || !b->timer.completed()) return ctx_fail(c, ADYPT_E_STATE, "adypt_get_rebuild_timing: nothing has been rebuilt yet (adypt_rebuild_bvh)");
	const int n = b->timer.read(ms, capacity, kTimingEvents - 1, true);
	if(b->last_ploc && capacity >= n) ms[3] = 0.0f; // (the rounds are entry [2]; there is no pass of its own behind them)
	return n;
}

int adypt_get_bvh_sizes(adypt_ctx *c, int64_t *n_nodes, int64_t *n_refs)
{
	if(!c) return ADYPT_E_INVALID;
	const CtxScene sc = ctx_scene(c);
	if(n_nodes) *n_nodes = sc.n_nodes;
	if(n_refs) *n_refs = sc.n_refs;
	return ADYPT_OK;
}

int adypt_read_tri_indices(adypt_ctx *c, int32_t *out)
{
	if(!c || !out) return ADYPT_E_INVALID;
	const CtxScene sc = ctx_scene(c);
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	if(sc.n_refs > 0) CTX_TRY(c, hipMemcpy(out, sc.tri_indices, (size_t)sc.n_refs * sizeof(int32_t), hipMemcpyDeviceToHost));
	return ADYPT_OK;
}

// the scene is replicated: the same rebuild on every device
int adypt_multi_rebuild_bvh(adypt_multi *m, const adypt_bvh_params *params, adypt_rebuild_info *out)
{
	// (bad parameters are refused by the first context: none has changed)
	return multi_each(m, [=](adypt_ctx *c) { return adypt_rebuild_bvh(c, params, out); });
}

int adypt_multi_rebuild_bvh_ploc(adypt_multi *m, const adypt_bvh_params *params, int radius, adypt_rebuild_info *out)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_rebuild_bvh_ploc(c, params, radius, out); });
}

int adypt_multi_rebuild_bvh_ploc_split(adypt_multi *m, const adypt_bvh_params *params, int radius, double split_budget, adypt_rebuild_info *out)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_rebuild_bvh_ploc_split(c, params, radius, split_budget, out); });
}

}  // extern "C"
