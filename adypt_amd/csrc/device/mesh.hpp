// Posing an indexed mesh by its vertices: THE definition of how an index buffer, one position per vertex and — given, or computed here — one normal per
// vertex become words 0..17 of every triangle record.  Compiled by the host (adypt_mesh_normals, adypt_mesh_triangles in host/mesh_host.cpp) and by
// the device (k_mesh_faces, k_mesh_normals, k_mesh_records in mesh.hip), which therefore give the same bits: no HIP needed, binary32 throughout, every
// operation in the written order, no fma (both compilers run with -ffp-contract=off), sqrtf and / the correctly rounded IEEE operations.  Restated in
// numpy as tests/mesh_truth.py.
//
//   binding         indices[3 t + c] in [0, n_vertices) is the vertex of corner c of triangle t; n_vertices in [1, 2^31 - 1].  A triangle may name one
//                   vertex twice; a vertex that no triangle names is allowed and never read.
//   incidence       vertex v's list holds the triangles t with indices[3 t + c] == v, once per such corner, in ascending 3 t + c: offsets
//                   (n_vertices + 1 values of 64 bits) into a list of 3 n_tris triangle indices, made by a counting pass (mesh_incidence).  The order
//                   is part of the definition: the sum below is taken in it.
//   face vector     e1[k] = p1[k] - p0[k], e2[k] = p2[k] - p0[k]; f[0] = e1[1] * e2[2] - e1[2] * e2[1], f[1] = e1[2] * e2[0] - e1[0] * e2[2],
//                   f[2] = e1[0] * e2[1] - e1[1] * e2[0]: two products and one difference each.  Area-weighted, oriented as the scene loader's flat normal.
//   computed normal acc = f(the list's first triangle), then acc[k] = acc[k] + f[k] for every later one in list order (an empty list: acc = +0);
//                   len2 = (acc.x * acc.x + acc.y * acc.y) + acc.z * acc.z; where len2 is a positive finite number n = acc / sqrtf(len2), otherwise
//                   n = acc as it is — pose_normal's rule.
//   given normals   used as given, not normalised (as adypt_update_triangles uses them).
//   record          corner c of triangle t, v = indices[3 t + c]: words 3 c .. 3 c + 2 are positions[v], words 9 + 3 c .. 9 + 3 c + 2 the normal of v.
//                   Words 18 and up keep their bytes.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#ifndef ADYPT_HOST_DEVICE
#ifdef __HIPCC__
#define ADYPT_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define ADYPT_HOST_DEVICE inline
#endif
#endif

namespace adypt {

constexpr int64_t kMeshMaxVertices = 2147483647;    // a vertex index is an int32

ADYPT_HOST_DEVICE void mesh_face(const float p0[3], const float p1[3], const float p2[3], float f[3])
{
	float e1[3], e2[3];
	for(int k = 0; k < 3; ++k) { e1[k] = p1[k] - p0[k]; e2[k] = p2[k] - p0[k]; }
	f[0] = e1[1] * e2[2] - e1[2] * e2[1];
	f[1] = e1[2] * e2[0] - e1[0] * e2[2];
	f[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// one more triangle of a vertex's list
ADYPT_HOST_DEVICE void mesh_accumulate(float acc[3], bool first, const float f[3])
{
	for(int k = 0; k < 3; ++k) acc[k] = first ? f[k] : acc[k] + f[k];
}

// the sum of a vertex's face vectors as its normal
ADYPT_HOST_DEVICE void mesh_normalise(const float acc[3], float n[3])
{
	const float len2 = (acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2];
	if(len2 > 0.0f && len2 < INFINITY)
	{
		const float s = sqrtf(len2);
		for(int k = 0; k < 3; ++k) n[k] = acc[k] / s;
	}
	else
		for(int k = 0; k < 3; ++k) n[k] = acc[k];
}

// ---- what a binding and a pose are refused for, on the host, before anything is touched: the reason, or null ----
// every one of n floats is finite: an exponent field that is not all ones.  No branch in the loop, so the compiler may take several floats at once —
// at pose time this pass is over every coordinate the caller gives
inline bool mesh_all_finite(const float *a, int64_t n)
{
	uint32_t bad = 0;
	for(int64_t i = 0; i < n; ++i)
	{
		uint32_t w;
		memcpy(&w, a + i, sizeof(w));
		bad |= (uint32_t)((w & 0x7f800000u) == 0x7f800000u);
	}
	return bad == 0;
}

// have_tris: the count the indices must be of (the context's; the host twins pass n_tris itself)
inline const char *mesh_refuse_counts(int64_t n_tris, int64_t have_tris, int64_t n_vertices)
{
	if(n_tris < 0 || n_tris != have_tris) return "n_tris is not the number of triangles the mesh is of";
	if(n_vertices < 1 || n_vertices > kMeshMaxVertices) return "n_vertices must be in [1, 2^31 - 1]";
	return nullptr;
}

inline const char *mesh_refuse_indices(const int32_t *indices, int64_t n_tris, int64_t n_vertices)
{
	for(int64_t i = 0; i < 3 * n_tris; ++i)
		if(indices[i] < 0 || (int64_t)indices[i] >= n_vertices) return "a vertex index is out of range";
	return nullptr;
}

// at pose time: n_vertices positions and, unless null, normals for a binding of bound_vertices
inline const char *mesh_refuse_pose(const float *positions, const float *normals, int64_t n_vertices, int64_t bound_vertices)
{
	if(n_vertices != bound_vertices) return "n_vertices is not the binding's";
	if(!mesh_all_finite(positions, 3 * n_vertices)) return "a position is not finite";
	if(normals && !mesh_all_finite(normals, 3 * n_vertices)) return "a given normal is not finite";
	return nullptr;
}

// The incidence lists of checked indices by a counting pass: offsets gets n_vertices + 1 values, list 3 n_tris triangle indices, vertex v's in
// ascending 3 t + c.  Returns the longest list's length.
inline int64_t mesh_incidence(const int32_t *indices, int64_t n_tris, int64_t n_vertices, std::vector<int64_t> &offsets, std::vector<int32_t> &list)
{
	offsets.assign((size_t)n_vertices + 1, 0);
	for(int64_t i = 0; i < 3 * n_tris; ++i) ++offsets[(size_t)indices[i] + 1];
	int64_t longest = 0;
	for(int64_t v = 0; v < n_vertices; ++v)
	{
		if(offsets[(size_t)v + 1] > longest) longest = offsets[(size_t)v + 1];
		offsets[(size_t)v + 1] += offsets[(size_t)v];
	}
	list.resize((size_t)(3 * n_tris));
	std::vector<int64_t> at(offsets.begin(), offsets.end() - 1);
	for(int64_t i = 0; i < 3 * n_tris; ++i) list[(size_t)at[(size_t)indices[i]]++] = (int32_t)(i / 3);
	return longest;
}

}  // namespace adypt
