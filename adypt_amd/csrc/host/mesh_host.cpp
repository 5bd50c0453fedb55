// adypt_mesh_normals, adypt_mesh_triangles, adypt_weld_triangles (include/adypt_host.h): an indexed mesh posed by its vertices, on the host, and the
// index buffer of a triangle soup.  The rule is ../device/mesh.hpp — the text the device path (mesh.hip) compiles too.
#include "common.hpp"
#include "../device/mesh.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

#include <unordered_map>

using namespace adypt;

namespace {

// what both entry points refuse of a mesh: the reason, or null
const char *mesh_refused(const int32_t *indices, int64_t n_tris, int64_t n_vertices, const float *positions, const float *normals_or_null)
{
	if(!indices || !positions) return "null argument";
	const char *why = mesh_refuse_counts(n_tris, n_tris, n_vertices);
	if(!why) why = mesh_refuse_indices(indices, n_tris, n_vertices);
	if(!why) why = mesh_refuse_pose(positions, normals_or_null, n_vertices, n_vertices);
	return why;
}

// everything has been checked
void computed_normals(const int32_t *indices, int64_t n_tris, int64_t n_vertices, const float *positions, float *normals_out)
{
	std::vector<float> faces((size_t)n_tris * 3);
	for(int64_t t = 0; t < n_tris; ++t)
	{
		const int32_t *ix = indices + 3 * t;
		mesh_face(positions + 3 * (size_t)ix[0], positions + 3 * (size_t)ix[1], positions + 3 * (size_t)ix[2], faces.data() + 3 * (size_t)t);
	}
	std::vector<int64_t> offsets;
	std::vector<int32_t> list;
	mesh_incidence(indices, n_tris, n_vertices, offsets, list);
	for(int64_t v = 0; v < n_vertices; ++v)
	{
		float acc[3] = {0.0f, 0.0f, 0.0f};
		for(int64_t k = offsets[(size_t)v]; k < offsets[(size_t)v + 1]; ++k) mesh_accumulate(acc, k == offsets[(size_t)v], faces.data() + 3 * (size_t)list[(size_t)k]);
		mesh_normalise(acc, normals_out + 3 * (size_t)v);
	}
}

// a corner's position and normal as bits
struct VertexKey {
	uint32_t w[6];
	bool operator==(const VertexKey &o) const { return !memcmp(w, o.w, sizeof(w)); }
};
struct VertexKeyHash {
	size_t operator()(const VertexKey &k) const
	{
		uint64_t h = 0xcbf29ce484222325ull;
		for(uint32_t x : k.w) { h ^= x; h *= 0x100000001b3ull; }
		return (size_t)(h ^ h >> 29);
	}
};

}  // namespace

int adypt_mesh_normals(const int32_t *indices, int64_t n_tris, int64_t n_vertices, const float *positions, float *normals_out)
{
	const char *why = normals_out ? mesh_refused(indices, n_tris, n_vertices, positions, nullptr) : "null argument";
	if(why) { set_host_error(std::string("adypt_mesh_normals: ") + why); return ADYPT_E_INVALID; }
	computed_normals(indices, n_tris, n_vertices, positions, normals_out);
	return ADYPT_OK;
}

int adypt_mesh_triangles(const void *triangles_in, int64_t n_tris, const int32_t *indices, int64_t n_vertices, const float *positions, const float *normals_or_null,
                         void *triangles_out)
{
	const char *why = triangles_in && triangles_out ? mesh_refused(indices, n_tris, n_vertices, positions, normals_or_null) : "null argument";
	if(why) { set_host_error(std::string("adypt_mesh_triangles: ") + why); return ADYPT_E_INVALID; }
	std::vector<float> computed;
	const float *normals = normals_or_null;
	if(!normals)
	{
		computed.resize((size_t)n_vertices * 3);
		computed_normals(indices, n_tris, n_vertices, positions, computed.data());
		normals = computed.data();
	}
	const uint8_t *in = (const uint8_t *)triangles_in;
	uint8_t *out = (uint8_t *)triangles_out;
	for(int64_t t = 0; t < n_tris; ++t)
	{
		TriRec r;
		memcpy(&r, in + t * sizeof(TriRec), sizeof(TriRec)); // (texture coordinates and material id stay)
		for(int c = 0; c < 3; ++c)
		{
			const size_t v = (size_t)indices[3 * t + c];
			r.p[c] = Vec3{positions[3 * v], positions[3 * v + 1], positions[3 * v + 2]};
			r.n[c] = Vec3{normals[3 * v], normals[3 * v + 1], normals[3 * v + 2]};
		}
		memcpy(out + t * sizeof(TriRec), &r, sizeof(TriRec));
	}
	return ADYPT_OK;
}

int64_t adypt_weld_triangles(const void *triangles, int64_t n_tris, int32_t *indices_out, float *positions_out, float *normals_out)
{
	if(!triangles || n_tris < 0 || 3 * n_tris > kMeshMaxVertices) { set_host_error("adypt_weld_triangles: null argument, or 3 n_tris outside [0, 2^31 - 1]"); return ADYPT_E_INVALID; }
	const uint8_t *in = (const uint8_t *)triangles;
	std::unordered_map<VertexKey, int32_t, VertexKeyHash> seen;
	seen.reserve((size_t)n_tris);
	for(int64_t t = 0; t < n_tris; ++t)
	{
		uint32_t w[18];
		memcpy(w, in + t * sizeof(TriRec), sizeof(w)); // p0 p1 p2 n0 n1 n2
		for(int c = 0; c < 3; ++c)
		{
			VertexKey k;
			memcpy(k.w, w + 3 * c, 12);
			memcpy(k.w + 3, w + 9 + 3 * c, 12);
			const auto at = seen.emplace(k, (int32_t)seen.size());
			const int32_t v = at.first->second;
			if(indices_out) indices_out[3 * t + c] = v;
			if(at.second && positions_out) memcpy(positions_out + 3 * (size_t)v, k.w, 12);
			if(at.second && normals_out) memcpy(normals_out + 3 * (size_t)v, k.w + 3, 12);
		}
	}
	return (int64_t)seen.size();
}
