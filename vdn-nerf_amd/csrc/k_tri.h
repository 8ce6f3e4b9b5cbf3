// Triangle helpers shared by the mesh evaluation and mesh cleaning kernels (mesh_eval.hip, mesh_clean.hip): corner indices of an
// int64 / int32 index buffer with the range check, and the area of a triangle in double from its fp32 vertices.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace vdn {

// corner indices of triangle f, or false when one of them is outside [0, V)
__device__ inline bool tri_corners(const void* triangles, int index_bytes, long V, long f, long* i) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        i[c] = index_bytes == 8 ? (long)((const int64_t*)triangles)[f * 3 + c] : (long)((const int32_t*)triangles)[f * 3 + c];
        if (i[c] < 0 || i[c] >= V) return false;
    }
    return true;
}

// 0.5 |(b - a) x (c - a)| in double (NaN / inf where a coordinate is: the callers test for it)
__device__ inline double tri_area(const float* vertices, const long* i) {
    double p[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) p[c][d] = (double)vertices[i[c] * 3 + d];
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

}  // namespace vdn
