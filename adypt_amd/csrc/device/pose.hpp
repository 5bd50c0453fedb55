// Posing triangles by matrices: THE definition of how a rest-pose triangle and a set of 3x4 matrices become the posed positions and normals.  Compiled by
// the host (adypt_pose_triangles in host/pose_host.cpp) and by the device (k_pose, pose.hip), which therefore give the same bits: no HIP needed,
// binary32 throughout, every operation in the written order, no fma (both compilers run with -ffp-contract=off), sqrtf and / the correctly rounded
// IEEE operations.  Restated in numpy as tests/pose_truth.py.
//
// A matrix B is 12 floats, row-major 3x4: B[4 r + 0..2] the linear part of row r, B[4 r + 3] its translation.
//   vertex matrix   parts: M = B[part].  Skin, slots k = 0..3 in order: the first slot with w_k != 0 gives M[j] = w_k * B_k[j], every later slot with
//                   w_k != 0 gives M[j] = M[j] + w_k * B_k[j]; a slot of weight 0 is skipped and its joint index never read; all four 0: M = 0.
//   position        p'[r] = ((M[r][0] * x + M[r][1] * y) + M[r][2] * z) + M[r][3]
//   normal          C = the cofactor matrix of M's 3x3 part (right under any affine map, mirrors included), every entry a * d - b * c as written;
//                   n'[r] = (C[r][0] * nx + C[r][1] * ny) + C[r][2] * nz; len2 = (n'x * n'x + n'y * n'y) + n'z * n'z; where len2 is a positive finite
//                   number n'[r] = n'[r] / sqrtf(len2), otherwise n' stays as it is.
//
// Morph targets (blend shapes) come before the matrices: rest pose -> morph -> vertex matrix -> record.  A morph layer has n_targets targets
// (1 .. 65536) and n_entries sparse entries (1 .. 2^31 - 1); an entry is (triangle, target, d[18]), d the deltas of words 0..17 of the triangle's
// record: p0 p1 p2, then n0 n1 n2.  A pose gives one weight per target, finite, of any sign, used as given.
//   morph stage     acc[0..17] starts as the rest pose's words 0..17.  The triangle's entries are taken in ascending target index, whatever order they
//                   were given in.  An entry whose weight w[target] == 0 is skipped and its deltas are never read: all weights 0 leave the rest pose's
//                   bits, a -0.0 included.  Every other entry does acc[j] = acc[j] + w * d[j], one product and one sum, each rounded.
//   matrix stage    vertex v goes through pose_vertex(M_v, acc + 3 v, acc + 9 + 3 v, ...) as without a layer.  The morphed normal is not normalised on
//                   its own: pose_normal normalises after the cofactor product.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#ifndef ADYPT_HOST_DEVICE
#ifdef __HIPCC__
#define ADYPT_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define ADYPT_HOST_DEVICE inline
#endif
#endif

namespace adypt {

constexpr int kPoseMatrixFloats = 12;
constexpr int kPoseSlots = 4;                       // weighted joints per vertex
constexpr int kPoseTriSlots = 3 * kPoseSlots;       // per triangle: vertex v's slot k at 4 v + k
constexpr int32_t kPoseMaxMatrices = 65536;         // a joint index is a uint16
enum PoseKind : int32_t { kPoseNone = 0, kPoseParts = 1, kPoseSkin = 2 };

// one slot of a skinned vertex, w != 0: M = w * B when it is the vertex's first, M + w * B after that
ADYPT_HOST_DEVICE void pose_weigh(float M[kPoseMatrixFloats], bool first, float w, const float B[kPoseMatrixFloats])
{
	for(int j = 0; j < kPoseMatrixFloats; ++j)
	{
		const float t = w * B[j];
		M[j] = first ? t : M[j] + t;
	}
}

constexpr int kMorphWords = 18;                     // an entry's deltas: words 0..17 of the record
constexpr int32_t kMorphMaxTargets = 65536;
constexpr int64_t kMorphMaxEntries = 2147483647;    // an offset is an int32

// one entry of weight w != 0
ADYPT_HOST_DEVICE void pose_morph(float acc[kMorphWords], float w, const float d[kMorphWords])
{
	for(int j = 0; j < kMorphWords; ++j)
	{
		const float t = w * d[j];
		acc[j] = acc[j] + t;
	}
}

ADYPT_HOST_DEVICE void pose_position(const float M[kPoseMatrixFloats], const float p[3], float out[3])
{
	for(int r = 0; r < 3; ++r) out[r] = ((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3];
}

// C[3 r + c] = A[r+1][c+1] * A[r+2][c+2] - A[r+1][c+2] * A[r+2][c+1], indices mod 3, A the 3x3 part of M
ADYPT_HOST_DEVICE void pose_cofactors(const float M[kPoseMatrixFloats], float C[9])
{
	for(int r = 0; r < 3; ++r)
	{
		const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
		for(int c = 0; c < 3; ++c)
		{
			const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
			C[3 * r + c] = M[4 * r1 + c1] * M[4 * r2 + c2] - M[4 * r1 + c2] * M[4 * r2 + c1];
		}
	}
}

ADYPT_HOST_DEVICE void pose_normal(const float C[9], const float n[3], float out[3])
{
	float t[3];
	for(int r = 0; r < 3; ++r) t[r] = (C[3 * r] * n[0] + C[3 * r + 1] * n[1]) + C[3 * r + 2] * n[2];
	const float len2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
	if(len2 > 0.0f && len2 < INFINITY)
	{
		const float s = sqrtf(len2);
		for(int r = 0; r < 3; ++r) t[r] = t[r] / s;
	}
	for(int r = 0; r < 3; ++r) out[r] = t[r];
}

// one vertex under its matrix
ADYPT_HOST_DEVICE void pose_vertex(const float M[kPoseMatrixFloats], const float p[3], const float n[3], float p_out[3], float n_out[3])
{
	float C[9];
	pose_cofactors(M, C);
	pose_position(M, p, p_out);
	pose_normal(C, n, n_out);
}

// ---- what a binding and a pose are refused for, on the host, before anything is touched: the reason, or null ----
inline bool pose_finite(float x) { return x - x == 0.0f; }

inline const char *pose_refuse_count(int64_t n_matrices)
{
	return n_matrices < 1 || n_matrices > kPoseMaxMatrices ? "the number of matrices must be in [1, 65536]" : nullptr;
}

inline const char *pose_refuse_parts(const int32_t *parts, int64_t n_tris, int64_t n_parts)
{
	for(int64_t i = 0; i < n_tris; ++i)
		if(parts[i] < 0 || parts[i] >= n_parts) return "a part index is out of range";
	return nullptr;
}

inline const char *pose_refuse_skin(const uint16_t *joints, const float *weights, int64_t n_tris, int64_t n_joints)
{
	for(int64_t i = 0; i < n_tris * kPoseTriSlots; ++i)
	{
		const float w = weights[i];
		if(!pose_finite(w) || w < 0.0f) return "a weight is negative or not finite";
		if(w != 0.0f && (int64_t)joints[i] >= n_joints) return "a joint index is out of range in a slot of non-zero weight";
	}
	return nullptr;
}

inline const char *pose_refuse_matrices(const float *matrices, int64_t n_matrices)
{
	for(int64_t i = 0; i < n_matrices * kPoseMatrixFloats; ++i)
		if(!pose_finite(matrices[i])) return "a matrix entry is not finite";
	return nullptr;
}


// ---- a morph layer ----
inline const char *pose_refuse_morph_counts(int64_t n_entries, int64_t n_targets)
{
	if(n_entries < 1 || n_entries > kMorphMaxEntries) return "the number of morph entries must be in [1, 2^31 - 1]";
	if(n_targets < 1 || n_targets > kMorphMaxTargets) return "the number of morph targets must be in [1, 65536]";
	return nullptr;
}

inline const char *pose_refuse_morph_entries(const int32_t *triangle_of_entry, const int32_t *target_of_entry, const float *deltas, int64_t n_entries, int64_t n_tris, int64_t n_targets)
{
	for(int64_t e = 0; e < n_entries; ++e)
	{
		if(triangle_of_entry[e] < 0 || triangle_of_entry[e] >= n_tris) return "a morph entry's triangle index is out of range";
		if(target_of_entry[e] < 0 || target_of_entry[e] >= n_targets) return "a morph entry's target index is out of range";
	}
	for(int64_t i = 0; i < n_entries * kMorphWords; ++i)
		if(!pose_finite(deltas[i])) return "a morph delta is not finite";
	return nullptr;
}

// The order the morph stage takes the entries in — by (triangle, target) — as indices into the arrays as given, and offsets[i] .. offsets[i + 1], the
// places of triangle i's entries in that order (n_tris + 1 values); the indices have been checked.  Refuses two entries of one (triangle, target).
inline const char *pose_morph_order(const int32_t *triangle_of_entry, const int32_t *target_of_entry, int64_t n_entries, int64_t n_tris, std::vector<int32_t> &order,
                                    std::vector<int32_t> &offsets)
{
	order.resize((size_t)n_entries);
	for(int64_t e = 0; e < n_entries; ++e) order[(size_t)e] = (int32_t)e;
	const auto key = [&](int32_t e) { return (int64_t)triangle_of_entry[e] * kMorphMaxTargets + target_of_entry[e]; };
	std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key(a) < key(b); });
	for(int64_t k = 1; k < n_entries; ++k)
		if(key(order[(size_t)k]) == key(order[(size_t)k - 1])) return "two morph entries have the same triangle and target";
	offsets.assign((size_t)n_tris + 1, 0);
	for(int64_t e = 0; e < n_entries; ++e) ++offsets[(size_t)triangle_of_entry[e] + 1];
	for(int64_t i = 0; i < n_tris; ++i) offsets[(size_t)i + 1] += offsets[(size_t)i];
	return nullptr;
}

// at pose time: `n_targets` weights given for a layer of `layer_targets` (0: no layer)
inline const char *pose_refuse_morph_weights(const float *morph_weights, int64_t n_targets, int64_t layer_targets)
{
	if(n_targets != layer_targets) return "the number of morph weights is not the layer's number of targets";
	for(int64_t k = 0; k < n_targets; ++k)
		if(!pose_finite(morph_weights[k])) return "a morph weight is not finite";
	return nullptr;
}

}  // namespace adypt
