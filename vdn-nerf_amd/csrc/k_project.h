// The "in image" rule shared by the mask votes and the visibility votes (mesh_clean.hip, mesh_ray.hip): one device function, so the
// two kernels cannot disagree about which cameras see a vertex.
#pragma once
#include <hip/hip_runtime.h>

namespace vdn {

// P [3][4] row-major maps (x, y, z) to (u w, v w, w), in double. True iff w > 0 and the pixel px = floor(u + 0.5), py = floor(v + 0.5)
// lies inside the H x W image; NaN and +-inf fail the range test (the comparisons are made in double, before any conversion to an
// integer). The contraction mode is pinned here, to the compiler's default, so that a file built with -ffp-contract=off
// (mesh_ray.hip) evaluates the projection as mesh_clean.hip does.
__device__ inline bool project_in_image(const double* P, double x, double y, double z, int H, int W, long* px_out, long* py_out) {
#pragma clang fp contract(fast)
    const double uw = P[0] * x + P[1] * y + P[2] * z + P[3], vw = P[4] * x + P[5] * y + P[6] * z + P[7],
                 w = P[8] * x + P[9] * y + P[10] * z + P[11];
    if (!(w > 0.0)) return false;
    const double px = floor(uw / w + 0.5), py = floor(vw / w + 0.5);
    if (!(px >= 0.0 && px < (double)W && py >= 0.0 && py < (double)H)) return false;
    *px_out = (long)px;
    *py_out = (long)py;
    return true;
}

}  // namespace vdn
