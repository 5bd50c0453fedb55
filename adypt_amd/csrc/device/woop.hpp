// The Woop matrix of a triangle reference (OglScene::init_triangles, src/Tracer/OglScene.cpp:93-116) and the 4x4 inverse it is made with.  ONE text
// for the host (adypt_woop_matrices, adypt_camera_matrices in host/host_api.cpp) and the device (k_refit_woop in refit.hip): no HIP needed, binary32,
// the operations in the order written, no fma (both sides are compiled with -ffp-contract=off).
#pragma once

#ifndef ADYPT_HOST_DEVICE
#ifdef __HIPCC__
#define ADYPT_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define ADYPT_HOST_DEVICE inline
#endif
#endif

namespace adypt {

// ---- glm::inverse(mat4) (dep/glm/detail/func_matrix.inl:294-351): cofactor expansion, column-major m[c*4+r] ----
ADYPT_HOST_DEVICE void inverse4(const float *a, float *out)
{
	auto m = [&](int c, int r) { return a[c * 4 + r]; };
	float c00 = m(2, 2) * m(3, 3) - m(3, 2) * m(2, 3), c02 = m(1, 2) * m(3, 3) - m(3, 2) * m(1, 3), c03 = m(1, 2) * m(2, 3) - m(2, 2) * m(1, 3);
	float c04 = m(2, 1) * m(3, 3) - m(3, 1) * m(2, 3), c06 = m(1, 1) * m(3, 3) - m(3, 1) * m(1, 3), c07 = m(1, 1) * m(2, 3) - m(2, 1) * m(1, 3);
	float c08 = m(2, 1) * m(3, 2) - m(3, 1) * m(2, 2), c10 = m(1, 1) * m(3, 2) - m(3, 1) * m(1, 2), c11 = m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2);
	float c12 = m(2, 0) * m(3, 3) - m(3, 0) * m(2, 3), c14 = m(1, 0) * m(3, 3) - m(3, 0) * m(1, 3), c15 = m(1, 0) * m(2, 3) - m(2, 0) * m(1, 3);
	float c16 = m(2, 0) * m(3, 2) - m(3, 0) * m(2, 2), c18 = m(1, 0) * m(3, 2) - m(3, 0) * m(1, 2), c19 = m(1, 0) * m(2, 2) - m(2, 0) * m(1, 2);
	float c20 = m(2, 0) * m(3, 1) - m(3, 0) * m(2, 1), c22 = m(1, 0) * m(3, 1) - m(3, 0) * m(1, 1), c23 = m(1, 0) * m(2, 1) - m(2, 0) * m(1, 1);
	const float f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11};
	const float f3[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
	const float v0[4] = {m(1, 0), m(0, 0), m(0, 0), m(0, 0)}, v1[4] = {m(1, 1), m(0, 1), m(0, 1), m(0, 1)};
	const float v2[4] = {m(1, 2), m(0, 2), m(0, 2), m(0, 2)}, v3[4] = {m(1, 3), m(0, 3), m(0, 3), m(0, 3)};
	float inv[4][4];
	for(int i = 0; i < 4; ++i)
	{
		const float sa = (i & 1) ? -1.0f : 1.0f, sb = -sa;
		inv[0][i] = (v1[i] * f0[i] - v2[i] * f1[i] + v3[i] * f2[i]) * sa;
		inv[1][i] = (v0[i] * f0[i] - v2[i] * f3[i] + v3[i] * f4[i]) * sb;
		inv[2][i] = (v0[i] * f1[i] - v1[i] * f3[i] + v3[i] * f5[i]) * sa;
		inv[3][i] = (v0[i] * f2[i] - v1[i] * f4[i] + v2[i] * f5[i]) * sb;
	}
	float det = (m(0, 0) * inv[0][0] + m(0, 1) * inv[1][0]) + (m(0, 2) * inv[2][0] + m(0, 3) * inv[3][0]);
	float ood = 1.0f / det;
	for(int c = 0; c < 4; ++c) for(int r = 0; r < 4; ++r) out[c * 4 + r] = inv[c][r] * ood;
}

// p: the triangle's three vertices (9 floats, p0 p1 p2); o: the 12 floats of its reference in the Woop array
ADYPT_HOST_DEVICE void woop_matrix(const float *p, float *o)
{
	const float e0x = p[0] - p[6], e0y = p[1] - p[7], e0z = p[2] - p[8];
	const float e1x = p[3] - p[6], e1y = p[4] - p[7], e1z = p[5] - p[8];
	const float nx = e0y * e1z - e1y * e0z, ny = e0z * e1x - e1z * e0x, nz = e0x * e1y - e1x * e0y;
	const float A[16] = {e0x, e1x, nx, p[6], e0y, e1y, ny, p[7], e0z, e1z, nz, p[8], 0.0f, 0.0f, 0.0f, 1.0f};
	float inv[16];
	inverse4(A, inv);
	o[0] = inv[8]; o[1] = inv[9]; o[2] = inv[10]; o[3] = -inv[11];
	for(int k = 0; k < 8; ++k) o[4 + k] = inv[k];
}

}  // namespace adypt
