// Posing an indexed mesh by its vertices on the device (include/adypt_hip.h adypt_bind_mesh, adypt_pose_vertices ...; the definition: mesh.hpp).  A
// translation unit of its own: nothing here is part of the tracer's code object.  A bind keeps, per context, the index buffer in three planes — plane c
// holds corner c of every triangle, so a wave's loads are 4 bytes per lane at neighbouring addresses — and the incidence lists the host made by a
// counting pass: 8-byte offsets per vertex and one triangle index per corner.  What one adypt_pose_vertices runs, all on the context's stream after the
// context has been drained:
//     the staging copies  12 B per vertex of positions and, when given, 12 B of normals, as they arrive: all that comes from the host
//     k_mesh_faces        (computed normals) one thread per triangle: three indices, three gathered positions, the face vector as one 16-byte store
//     k_mesh_normals      (computed normals) one thread per vertex: its two offsets, then its list in order — a variable trip count, lanes diverge — the
//                         face vectors added in list order and normalised.  No atomics and no reduction across lanes: the order of the sum is the definition.
//     k_mesh_records      one thread per triangle: three indices, three gathered positions and normals, words 0..17 of the record written as k_pose
//                         writes them: four 16-byte stores and one of 8 bytes for words 16 and 17.  A pose never reads the records.
//     (refit.hip)         the refit's tail, refit_tail: per-reference copy, Woop data, node levels, root card, reset
// The copies and the three kernels stand between timer marks of their own (adypt_get_mesh_timing); together they are the first stage of
// adypt_get_refit_timing.
#include "ctx_unit.hpp"
#include "mesh.hpp"
#include "mesh_internal.hpp"
#include "refit_internal.hpp"
#include "tri_record.hpp"
#include "../../../include/adypt_hip.h"

#include <string>
#include <vector>

using namespace adypt;

namespace {

constexpr int kMeshThreads = 256;
constexpr int kMeshBatch = 8;                               // k_mesh_normals: entries of a vertex's list whose loads are in flight together
constexpr int kMeshStages = 4;                             // adypt_get_mesh_timing: the upload, k_mesh_faces, k_mesh_normals, k_mesh_records
static_assert(kTriRecordWords == 32, "the record of tri_record.hpp");

// a vertex's three floats from an array of 12 bytes per vertex
__device__ __forceinline__ void load3(const float *__restrict__ a, int32_t v, float out[3])
{
	const float *p = a + 3 * (size_t)(uint32_t)v;
	out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
}

// indices: three planes of n.  Every index has been checked on the host (mesh.hpp, mesh_refuse_*).
__global__ __launch_bounds__(kMeshThreads) void k_mesh_faces(const int32_t *__restrict__ indices, int64_t n, const float *__restrict__ positions, float4 *__restrict__ faces)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const size_t at = (size_t)i, plane = (size_t)n;
	float p0[3], p1[3], p2[3], f[3];
	load3(positions, indices[at], p0);
	load3(positions, indices[plane + at], p1);
	load3(positions, indices[2 * plane + at], p2);
	mesh_face(p0, p1, p2, f);
	faces[at] = make_float4(f[0], f[1], f[2], 0.0f);
}

// offsets: n_vertices + 1 places into list, whose entries are triangle indices below the number of faces
__global__ __launch_bounds__(kMeshThreads) void k_mesh_normals(const int64_t *__restrict__ offsets, const int32_t *__restrict__ list, int64_t n_vertices,
                                                                const float4 *__restrict__ faces, float *__restrict__ normals)
{
	const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(v >= n_vertices) return;
	const int64_t begin = offsets[v], end = offsets[v + 1];
	float acc[3] = {0.0f, 0.0f, 0.0f};
	// kMeshBatch entries at a time: their indices, then their face vectors, are loaded before the first is added, so a long list (a fan's apex) waits
	// for memory twice per batch and not twice per entry; the additions stay one by one, in list order.  Nothing between the loads and the last
	// addition is a branch — an entry past the list's end names triangle 0 and is added by a select that keeps acc — so the loads cannot sink
	// behind one another's waits
	for(int64_t k = begin; k < end; k += kMeshBatch)
	{
		int32_t t[kMeshBatch];
		float4 f4[kMeshBatch];
#pragma unroll
		for(int j = 0; j < kMeshBatch; ++j) t[j] = k + j < end ? list[k + j] : 0; // (triangle 0 exists; its face vector is not added)
#pragma unroll
		for(int j = 0; j < kMeshBatch; ++j) f4[j] = faces[(size_t)(uint32_t)t[j]];
#pragma unroll
		for(int j = 0; j < kMeshBatch; ++j)
		{
			const bool live = k + j < end;
			const float f[3] = {f4[j].x, f4[j].y, f4[j].z};
			float next[3] = {acc[0], acc[1], acc[2]};
			mesh_accumulate(next, k + j == begin, f);
#pragma unroll
			for(int c = 0; c < 3; ++c) acc[c] = live ? next[c] : acc[c];
		}
	}
	float nrm[3];
	mesh_normalise(acc, nrm);
	float *out = normals + 3 * (size_t)v;
	out[0] = nrm[0]; out[1] = nrm[1]; out[2] = nrm[2];
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_records(float4 *records, int tri_float4, const int32_t *__restrict__ indices, int64_t n,
                                                                const float *__restrict__ positions, const float *__restrict__ normals)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const size_t at = (size_t)i, plane = (size_t)n;
	float out[18];
#pragma unroll
	for(int c = 0; c < 3; ++c)
	{
		const int32_t v = indices[(size_t)c * plane + at];
		load3(positions, v, out + 3 * c);
		load3(normals, v, out + 9 + 3 * c);
	}
	float4 *rec = records + at * (size_t)tri_float4;
	rec[0] = make_float4(out[0], out[1], out[2], out[3]);
	rec[1] = make_float4(out[4], out[5], out[6], out[7]);
	rec[2] = make_float4(out[8], out[9], out[10], out[11]);
	rec[3] = make_float4(out[12], out[13], out[14], out[15]);
	((float2 *)rec)[8] = make_float2(out[16], out[17]); // (words 18, 19 — material id, class word — share this vector and keep their bytes)
}

// what a bind leaves on the device
struct Binding {
	int64_t n_vertices = 0, n_tris = 0;
	int32_t max_valence = 0;
	bool posed = false;       // `normals` holds those of a pose: adypt_read_vertex_normals answers
	Buffer<int32_t> indices;  // 3 planes of n_tris: 12 B per triangle
	Buffer<int32_t> list;     // the incidence lists: 12 B per triangle
	Buffer<int64_t> offsets;  // n_vertices + 1
	Buffer<float4> faces;     // the face vectors of the last pose with computed normals: 16 B per triangle
	Buffer<float> positions;  // the staging buffer of the positions: 12 B per vertex
	Buffer<float> normals;    // the normals, staged or computed: 12 B per vertex
	int64_t device_bytes() const { return (int64_t)(indices.bytes() + list.bytes() + offsets.bytes() + faces.bytes() + positions.bytes() + normals.bytes()); }
};

// kept per context
struct Mesher {
	Binding bound;
	StageTimer<kMeshStages + 1> timer; // the stages of the last pose: marks 0 .. 4 around the four of them with computed normals; with given normals
	bool given = false;                // marks 0 .. 2 around the upload and k_mesh_records, nothing being between the two
};

// the refit whose writers are the mesh kernels
int pose_and_refit(adypt_ctx *c, Mesher &m, const float *positions, const float *normals)
{
	Binding &b = m.bound;
	CTX_STEP(refit_begin(c));
	const CtxInfo i = ctx_info(c);
	const CtxScene sc = ctx_scene(c);
	const size_t bytes = (size_t)b.n_vertices * 3 * sizeof(float);
	b.posed = false;
	m.timer.invalidate();
	CTX_TRY(c, m.timer.mark(0, i.stream));
	CTX_TRY(c, hipMemcpyAsync(b.positions.get(), positions, bytes, hipMemcpyHostToDevice, i.stream));
	if(normals) CTX_TRY(c, hipMemcpyAsync(b.normals.get(), normals, bytes, hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, m.timer.mark(1, i.stream));
	m.given = normals != nullptr;
	if(!normals)
	{
		hipLaunchKernelGGL(k_mesh_faces, dim3(grid_of(b.n_tris, kMeshThreads)), dim3(kMeshThreads), 0, i.stream, (const int32_t *)b.indices.get(), b.n_tris,
		                   (const float *)b.positions.get(), b.faces.get());
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, m.timer.mark(2, i.stream));
		hipLaunchKernelGGL(k_mesh_normals, dim3(grid_of(b.n_vertices, kMeshThreads)), dim3(kMeshThreads), 0, i.stream, (const int64_t *)b.offsets.get(),
		                   (const int32_t *)b.list.get(), b.n_vertices, (const float4 *)b.faces.get(), b.normals.get());
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, m.timer.mark(3, i.stream));
	}
	hipLaunchKernelGGL(k_mesh_records, dim3(grid_of(b.n_tris, kMeshThreads)), dim3(kMeshThreads), 0, i.stream, sc.triangles, sc.tri_float4, (const int32_t *)b.indices.get(),
	                   b.n_tris, (const float *)b.positions.get(), (const float *)b.normals.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, m.timer.mark(m.given ? 2 : 4, i.stream));
	CTX_STEP(refit_tail(c));
	m.timer.complete(); // (the tail has waited for the stream)
	b.posed = true;
	return ADYPT_OK;
}

// the context's state where its binding is of the context's triangles, else null with the context's error set
Mesher *bound_mesh(adypt_ctx *c, const char *who, int *code)
{
	Mesher *ms = ctx_state_if_any<Mesher>(c, kAttachMesh);
	if(!ms || ms->bound.n_vertices == 0) { *code = ctx_fail(c, ADYPT_E_STATE, std::string(who) + ": no mesh binding (adypt_bind_mesh; adypt_set_triangles drops it)"); return nullptr; }
	if(ms->bound.n_tris != ctx_scene(c).n_tris) { *code = ctx_fail(c, ADYPT_E_STATE, std::string(who) + ": the mesh binding is not of the context's triangles"); return nullptr; }
	return ms;
}

}  // namespace

namespace adypt {

void mesh_drop_binding(adypt_ctx *c)
{
	Mesher *ms = ctx_state_if_any<Mesher>(c, kAttachMesh);
	if(ms) ms->bound = Binding();
}

}  // namespace adypt

extern "C" {

int adypt_bind_mesh(adypt_ctx *c, const int32_t *indices, int64_t n_tris, int64_t n_vertices)
{
	if(!c) return ADYPT_E_INVALID;
	const std::string who = "adypt_bind_mesh: ";
	if(!indices) return ctx_fail(c, ADYPT_E_INVALID, who + "null argument");
	const int64_t n = ctx_scene(c).n_tris;
	const char *r = mesh_refuse_counts(n_tris, n, n_vertices);
	if(!r) r = mesh_refuse_indices(indices, n_tris, n_vertices);
	if(r) return ctx_fail(c, ADYPT_E_INVALID, who + r);
	if(ctx_scene(c).tri_float4 * 4 != kTriRecordWords) return ctx_fail(c, ADYPT_E_HIP, who + "the record layout is not tri_record.hpp's");
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	// the indices in planes, the incidence lists
	std::vector<int32_t> planes((size_t)n * 3), list;
	std::vector<int64_t> offsets;
	for(int64_t t = 0; t < n; ++t)
		for(int k = 0; k < 3; ++k) planes[(size_t)k * (size_t)n + (size_t)t] = indices[3 * t + k];
	const int64_t longest = mesh_incidence(indices, n, n_vertices, offsets, list);
	// the new binding is complete before it takes the place of the old one: a failure leaves the old one in place
	Binding nb;
	nb.n_vertices = n_vertices; nb.n_tris = n; nb.max_valence = (int32_t)std::min<int64_t>(longest, INT32_MAX);
	CTX_TRY(c, at_least(nb.indices, planes.size()));
	CTX_TRY(c, at_least(nb.list, list.size()));
	CTX_TRY(c, at_least(nb.offsets, offsets.size()));
	CTX_TRY(c, at_least(nb.faces, (size_t)n));
	CTX_TRY(c, at_least(nb.positions, (size_t)n_vertices * 3));
	CTX_TRY(c, at_least(nb.normals, (size_t)n_vertices * 3));
	CTX_TRY(c, hipMemcpyAsync(nb.indices.get(), planes.data(), planes.size() * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipMemcpyAsync(nb.list.get(), list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipMemcpyAsync(nb.offsets.get(), offsets.data(), offsets.size() * sizeof(int64_t), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	ctx_state<Mesher>(c, kAttachMesh)->bound = std::move(nb); // (the old binding's memory goes with `nb`)
	return ADYPT_OK;
}

int adypt_pose_vertices(adypt_ctx *c, const float *positions, const float *normals, int64_t n_vertices, const adypt_bvh_params *params, const adypt_pose_policy *policy,
                        adypt_pose_outcome *outcome)
{
	if(!c) return ADYPT_E_INVALID;
	const char *who = "adypt_pose_vertices";
	if(!positions) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": positions is null");
	int code = ADYPT_OK;
	Mesher *m = bound_mesh(c, who, &code);
	if(!m) return code;
	const Binding *b = &m->bound;
	if(const char *r = mesh_refuse_pose(positions, normals, n_vertices, b->n_vertices)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": " + r);
	if(!policy)
	{
		CTX_TRY(c, hipSetDevice(ctx_info(c).device));
		CTX_STEP(pose_and_refit(c, *m, positions, normals));
		if(outcome) *outcome = adypt_pose_outcome{};
		return ADYPT_OK;
	}
	BuildRequest request;
	if(const char *why = refit_policy_refused(params, policy, &request)) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": " + why);
	return refit_under_policy(c, who, request, policy->rebuild_above, outcome, [&]() { return pose_and_refit(c, *m, positions, normals); });
}

int adypt_read_vertex_normals(adypt_ctx *c, float *normals)
{
	if(!c) return ADYPT_E_INVALID;
	const char *who = "adypt_read_vertex_normals";
	if(!normals) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": normals is null");
	int code = ADYPT_OK;
	Mesher *m = bound_mesh(c, who, &code);
	if(!m) return code;
	const Binding *b = &m->bound;
	if(!b->posed) return ctx_fail(c, ADYPT_E_STATE, std::string(who) + ": no adypt_pose_vertices since the bind");
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipMemcpyAsync(normals, b->normals.get(), (size_t)b->n_vertices * 3 * sizeof(float), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	return ADYPT_OK;
}

int adypt_get_mesh_timing(adypt_ctx *c, float *ms, int capacity)
{
	if(!c) return ADYPT_E_INVALID;
	if(!ms) return ctx_fail(c, ADYPT_E_INVALID, "adypt_get_mesh_timing: ms is null");
	Mesher *m = ctx_state_if_any<Mesher>(c, kAttachMesh);
	if(!m || !m->timer.completed()) return ctx_fail(c, ADYPT_E_STATE, "adypt_get_mesh_timing: no vertex pose yet (adypt_pose_vertices)");
	if(!m->given) return m->timer.read(ms, capacity, kMeshStages, false);
	if(capacity < kMeshStages) return kMeshStages;
	float two[2] = {0.0f, 0.0f}; // (given normals: the upload and k_mesh_records; the two kernels between them did not run)
	(void)m->timer.read(two, 2, 2, false);
	ms[0] = two[0]; ms[1] = 0.0f; ms[2] = 0.0f; ms[3] = two[1];
	return kMeshStages;
}

int adypt_unbind_mesh(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	CTX_TRY(c, hipSetDevice(ctx_info(c).device));
	CTX_STEP(ctx_drain(c));
	mesh_drop_binding(c);
	return ADYPT_OK;
}

int adypt_get_mesh_binding(adypt_ctx *c, adypt_mesh_binding *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, "adypt_get_mesh_binding: out is null");
	const Mesher *ms = ctx_state_if_any<Mesher>(c, kAttachMesh);
	*out = adypt_mesh_binding{};
	if(ms && ms->bound.n_vertices > 0) *out = adypt_mesh_binding{ms->bound.n_vertices, ms->bound.n_tris, ms->bound.max_valence, ms->bound.device_bytes()};
	return ADYPT_OK;
}

// the scene is replicated: the same binding and the same pose on every device
int adypt_multi_bind_mesh(adypt_multi *m, const int32_t *indices, int64_t n_tris, int64_t n_vertices)
{
	// (bad arguments are refused by the first context: none has changed)
	return multi_each(m, [=](adypt_ctx *c) { return adypt_bind_mesh(c, indices, n_tris, n_vertices); });
}

int adypt_multi_pose_vertices(adypt_multi *m, const float *positions, const float *normals, int64_t n_vertices, const adypt_bvh_params *params, const adypt_pose_policy *policy,
                              adypt_pose_outcome *outcome)
{
	return multi_each_outcome(m, "adypt_multi_pose_vertices", outcome,
	                          [=](adypt_ctx *c, adypt_pose_outcome *o) { return adypt_pose_vertices(c, positions, normals, n_vertices, params, policy, o); });
}

// every device holds the same normals: the first one's
int adypt_multi_read_vertex_normals(adypt_multi *m, float *normals)
{
	int k = 0;
	return multi_each(m, [&](adypt_ctx *c) { return k++ == 0 ? adypt_read_vertex_normals(c, normals) : (int)ADYPT_OK; });
}

int adypt_multi_unbind_mesh(adypt_multi *m)
{
	return multi_each(m, [](adypt_ctx *c) { return adypt_unbind_mesh(c); });
}

// every device holds the same binding: the first one's
int adypt_multi_get_mesh_binding(adypt_multi *m, adypt_mesh_binding *out)
{
	if(m && !out) { multi_set_error(m, "adypt_multi_get_mesh_binding: out is null"); return ADYPT_E_INVALID; }
	int k = 0;
	return multi_each(m, [&](adypt_ctx *c) {
		adypt_mesh_binding b{};
		CTX_STEP(adypt_get_mesh_binding(c, &b));
		if(k++ == 0) *out = b;
		return (int)ADYPT_OK;
	});
}

}  // extern "C"
