// Texel colours from the training photographs (include/vdn_render.h: vdn_tex_photo; vdn_hip/mesh.py: photo_colors, bake_texture(photos=);
// DESIGN.md 3t). One thread per texel point walks the cameras in index order: in front, in frame, facing, and - last, the only test
// that walks the grid - unoccluded (k_ray_grid.h: the any-hit walk of vdn_visibility_votes, ignoring the texel's own face). No
// atomics: every sum has one order, so two runs and two cell sizes give the same bits. Built with -ffp-contract=off: every product and
// sum is rounded on its own, in the order the header states, and a numpy fp64 restatement gives the same decisions and sums.
// Texels are face-major, so the lanes of a wave hold neighbouring points; they visit camera k in the same iteration and their
// segments walk the same cells. P_mat and centres are indexed by k only (wave-uniform: scalar loads).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cmath>
#include "vdn_render.h"
#include "k_ray_grid.h"

namespace vdn {

__global__ void __launch_bounds__(256) tex_photo_kernel(VdnTexPhotoArgs a) {
    const RayGrid g = ray_grid(a);
    const double* __restrict__ Pm = a.P_mat;
    const double* __restrict__ centres = a.centres;
    const float* __restrict__ images = a.images;
    const float4* records = (const float4*)a.records;
    const long H = a.H, W = a.W;
    const double w_edge = (double)(a.W - 1), h_edge = (double)(a.H - 1);
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < (long)a.P; p += stride) {
        double sum_w = 0.0, sum_c[3] = {0.0, 0.0, 0.0}, best_w = 0.0, best_c[3] = {0.0, 0.0, 0.0};
        int n_views = 0, best = -1;
        const long f = (long)a.face[p];
        bool live = f >= 0 && f < (long)a.F;
        if (!live) *a.error = 1;                                   // (every writer stores the same word)
        const double x = (double)a.points[p * 3], y = (double)a.points[p * 3 + 1], z = (double)a.points[p * 3 + 2];
        const float* an = a.anchors != nullptr ? a.anchors : a.points;
        const double ax = (double)an[p * 3], ay = (double)an[p * 3 + 1], az = (double)an[p * 3 + 2];
        // the unit normal: the given row (one-sided), or the face's own from the grid's record (two-sided)
        double nx = 0.0, ny = 0.0, nz = 0.0;
        const bool two_sided = a.normals == nullptr;
        if (live) {
            if (!two_sided) {
                nx = (double)a.normals[p * 3], ny = (double)a.normals[p * 3 + 1], nz = (double)a.normals[p * 3 + 2];
            } else {
                const float4 r0 = records[f * 3], r1 = records[f * 3 + 1], r2 = records[f * 3 + 2];
                const double e1x = (double)r0.w - (double)r0.x, e1y = (double)r1.x - (double)r0.y, e1z = (double)r1.y - (double)r0.z;
                const double e2x = (double)r1.z - (double)r0.x, e2y = (double)r1.w - (double)r0.y, e2z = (double)r2.x - (double)r0.z;
                nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            }
            const double len = sqrt((nx * nx + ny * ny) + nz * nz);
            live = len > 0.0 && len < INFINITY;                   // (a zero or non-finite normal sees no camera)
            nx = nx / len, ny = ny / len, nz = nz / len;
        }
        for (long k = 0; live && k < (long)a.N; ++k) {
            const double* M = Pm + k * 12;
            // 1. in front
            const double uw = ((M[0] * x + M[1] * y) + M[2] * z) + M[3], vw = ((M[4] * x + M[5] * y) + M[6] * z) + M[7],
                         w = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
            if (!(w > 0.0)) continue;
            const double u = uw / w, v = vw / w;
            // 2. in frame (each comparison fails on NaN, so the min below sees none)
            const double ur = w_edge - u, vr = h_edge - v;
            if (!(u >= 0.0 && ur >= 0.0 && v >= 0.0 && vr >= 0.0)) continue;
            const double m = fmin(fmin(u, ur), fmin(v, vr));
            const double border = a.feather > 0.0 ? fmin(1.0, m / a.feather) : 1.0;
            // 3. facing
            const double o[3] = {centres[k * 3], centres[k * 3 + 1], centres[k * 3 + 2]};
            const double rx = o[0] - x, ry = o[1] - y, rz = o[2] - z;
            double cs = ((nx * rx + ny * ry) + nz * rz) / sqrt((rx * rx + ry * ry) + rz * rz);
            if (two_sided) cs = fmax(cs, -cs);
            if (!(cs > a.cos_min)) continue;
            const double wk = (cs * cs) * border;
            if (!(wk > 0.0)) continue;
            // 4. unoccluded: nothing but the texel's own face between the camera and the texel's place on its triangle
            const double d[3] = {ax - o[0], ay - o[1], az - o[2]};
            if (cast_ray<true>(g, o, d, 0.0, 1.0 - a.eps, -1, f).face >= 0) continue;
            // the bilinear value of image k at (u, v): pixel centres at integer coordinates
            const double fx0 = floor(u), fy0 = floor(v);
            const long x0 = (long)fx0, y0 = (long)fy0, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
            const double tx = u - fx0, ty = v - fy0;
            const double w00 = (1.0 - tx) * (1.0 - ty), w10 = tx * (1.0 - ty), w01 = (1.0 - tx) * ty, w11 = tx * ty;
            const float* img = images + k * H * W * 3;
            const float *t00 = img + (y0 * W + x0) * 3, *t10 = img + (y0 * W + x1) * 3, *t01 = img + (y1 * W + x0) * 3, *t11 = img + (y1 * W + x1) * 3;
            const bool better = wk > best_w;                       // (strictly: the lower index wins ties)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double col = (w00 * (double)t00[c] + w10 * (double)t10[c]) + (w01 * (double)t01[c] + w11 * (double)t11[c]);
                sum_c[c] = sum_c[c] + wk * col;
                if (better) best_c[c] = col;
            }
            sum_w = sum_w + wk;
            if (better) best_w = wk, best = (int)k;
            ++n_views;
        }
        float out[3] = {0.f, 0.f, 0.f}, weight = 0.f;
        if (n_views > 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = (float)(a.blend != 0 ? best_c[c] : sum_c[c] / sum_w);
            weight = (float)(a.blend != 0 ? best_w : sum_w);
        }
        a.colors[p * 3] = out[0], a.colors[p * 3 + 1] = out[1], a.colors[p * 3 + 2] = out[2];
        a.weight[p] = weight;
        a.n_views[p] = n_views;
        a.best_view[p] = best;
    }
}

}  // namespace vdn

extern "C" int vdn_tex_photo(const VdnTexPhotoArgs* a, void* stream) {
    if (a == nullptr || a->points == nullptr || a->face == nullptr || a->P_mat == nullptr || a->centres == nullptr || a->images == nullptr ||
        a->records == nullptr || a->cell_start == nullptr || a->refs == nullptr || a->colors == nullptr || a->weight == nullptr ||
        a->n_views == nullptr || a->best_view == nullptr || a->error == nullptr || a->P < 1 || a->N < 1 || a->F < 1 || a->n_refs < 0 ||
        a->H < 1 || a->W < 1 || (a->blend != 0 && a->blend != 1) || !(a->cos_min >= 0.0 && a->cos_min < 1.0) ||
        !(a->feather >= 0.0 && a->feather < INFINITY) || !(a->eps >= 0.0 && a->eps < 1.0) ||
        !geometry_ok(a->nx, a->ny, a->nz, a->lo_x, a->lo_y, a->lo_z, a->h, a->margin)) return -1;
    if (a->P > INT_MAX || a->N > INT_MAX || a->F > INT_MAX || a->n_refs > INT_MAX || cell_total(a->nx, a->ny, a->nz) < 0) return -10;
    hipLaunchKernelGGL(vdn::tex_photo_kernel, dim3(grid_of(a->P)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
