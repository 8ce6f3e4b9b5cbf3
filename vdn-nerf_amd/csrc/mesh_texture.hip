// Textured meshes on the device (include/vdn_render.h: vdn_tex_points, vdn_tex_project, vdn_tex_gather, vdn_tex_sample; vdn_hip/mesh.py:
// bake_texture and its parts). Every face owns a right-triangle patch of a per-face atlas, two faces to a square cell.
// Four element-wise passes: the surface point of every owned texel, one Newton step of those points towards the level set, the
// atlas gathered texel by texel from the shaded colours, and a bilinear lookup at points of the surface. The layout is integer
// arithmetic, restated here from the header; the positions and the lookup are double on double vertices, and the file is built with
// -ffp-contract=off, so every product and sum rounds on its own and a numpy model can follow them. Memory-bound, wave64, a flat
// grid, no LDS, no atomics: every output byte is written once.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include "vdn_render.h"
#include "k_tri.h"

namespace vdn {

// first r of row j of a half's enumeration: rows j = 0 .. n - 2 hold n - 1 - j texels
__device__ inline long tex_row_start(long n, long j) { return j * (2 * n - 1 - j) / 2; }

// r -> (i, j): the largest j whose row starts at or before r, from the root of the quadratic and corrected by whole steps
__device__ inline void tex_unrank(long n, long r, long* i, long* j) {
    const double b = (double)(2 * n - 1);
    long jj = (long)floor(0.5 * (b - sqrt(b * b - 8.0 * (double)r)));
    if (jj < 0) jj = 0;
    if (jj > n - 2) jj = n - 2;
    while (jj > 0 && tex_row_start(n, jj) > r) --jj;
    while (jj < n - 2 && tex_row_start(n, jj + 1) <= r) ++jj;
    *j = jj;
    *i = r - tex_row_start(n, jj);
}

__global__ void tex_points_kernel(VdnTexArgs a) {
    const long n = a.n, m = n - 3, T = n * (n - 1) / 2, P = (long)a.F * T;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < P; q += stride) {
        const long f = q / T;
        long i, j, c[3];
        tex_unrank(n, q - f * T, &i, &j);
        double p[3] = {0.0, 0.0, 0.0};
        if (!tri_corners(a.triangles, a.index_bytes, (long)a.V, f, c)) {
            *a.error = 1;                                           // (every writer stores the same word)
        } else {
            double b0, b1, b2;
            if (i + j <= m) {
                b1 = (double)i / (double)m;
                b2 = (double)j / (double)m;
                b0 = (1.0 - b1) - b2;
            } else {                                                // the gutter: the nearest point of the hypotenuse
                b1 = fmin(fmax(((double)i - 0.5) / (double)m, 0.0), 1.0);
                b2 = 1.0 - b1;
                b0 = 0.0;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
                p[k] = (b0 * a.vertices[c[0] * 3 + k] + b1 * a.vertices[c[1] * 3 + k]) + b2 * a.vertices[c[2] * 3 + k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.points[q * 3 + k] = (float)p[k];
        a.face[q] = (int32_t)f;
    }
}

__device__ inline float step_towards(float y, float target) { return y == target ? y : nextafterf(y, target); }

__global__ void tex_project_kernel(VdnTexProjectArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < (long)a.N; p += stride) {
        const float xf[3] = {a.x[p * 3 + 0], a.x[p * 3 + 1], a.x[p * 3 + 2]};
        const double c[3] = {(double)a.x0[p * 3 + 0], (double)a.x0[p * 3 + 1], (double)a.x0[p * 3 + 2]};
        const double g[3] = {(double)a.g[p * 3 + 0], (double)a.g[p * 3 + 1], (double)a.g[p * 3 + 2]};
        const double s = (double)a.sdf[p];
        const double den = fmax((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2], 1e-12);
        double y[3], e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            y[k] = (double)xf[k] + (-s * g[k]) / den;
            e[k] = y[k] - c[k];
        }
        const double r = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        if (r > a.max_offset) {
            const double w = a.max_offset / r;
#pragma unroll
            for (int k = 0; k < 3; ++k) y[k] = c[k] + e[k] * w;
        }
        float o[3] = {(float)y[0], (float)y[1], (float)y[2]};
        const double d0 = (double)o[0] - c[0], d1 = (double)o[1] - c[1], d2 = (double)o[2] - c[2];
        if (sqrt((d0 * d0 + d1 * d1) + d2 * d2) > a.max_offset) {    // the rounding to fp32 carried the point out of the ball
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = step_towards(o[k], a.x0[p * 3 + k]);
        }
        // (g is tested on its own: a NaN in it is lost in fmax(., 1e-12) and an inf can cancel to a finite step)
        const bool ok = isfinite(s) && isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) a.out[p * 3 + k] = ok ? o[k] : xf[k];
    }
}

__device__ inline uint8_t tex_byte(float c) { return (uint8_t)rintf(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f); }

__global__ void tex_gather_kernel(VdnTexArgs a) {
    const long S = a.S, n = a.n, C = S / n, T = n * (n - 1) / 2, N = S * S;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += stride) {
        const long x = t % S, y = t / S, cx = x / n, cy = y / n;
        long q = -1;                                                // the texel point this texel shows, or none
        if (cx < C && cy < C) {
            const long c = cy * C + cx;
            long i = x - cx * n, j = y - cy * n, f = 2 * c;
            if (i + j == n - 1) {                                   // the diagonal repeats a gutter texel of the lower half
                if (j > 0) --j;
                else --i;
            } else if (i + j >= n) {                                // the upper half, turned by 180 degrees
                i = n - 1 - i;
                j = n - 1 - j;
                f = 2 * c + 1;
            }
            if (f < (long)a.F) q = f * T + tex_row_start(n, j) + i;
        }
        uint8_t r = 0, g = 0, b = 0;
        if (q >= 0) {
            b = tex_byte(a.colors[q * 3 + 0]);
            g = tex_byte(a.colors[q * 3 + 1]);
            r = tex_byte(a.colors[q * 3 + 2]);
        }
        a.atlas[t * 3 + 0] = r;
        a.atlas[t * 3 + 1] = g;
        a.atlas[t * 3 + 2] = b;
    }
}

__global__ void tex_sample_kernel(VdnTexArgs a) {
    const long S = a.S, n = a.n, C = S / n;
    const double m = (double)(n - 3);
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < (long)a.R; p += stride) {
        const long f = (long)a.hit_face[p];
        long c[3];
        bool hit = f >= 0 && f < (long)a.F;
        if (hit && !tri_corners(a.triangles, a.index_bytes, (long)a.V, f, c)) {
            *a.error = 1;
            hit = false;
        }
        if (!hit) {
            a.rgb[p * 3 + 0] = (float)a.bg_r;
            a.rgb[p * 3 + 1] = (float)a.bg_g;
            a.rgb[p * 3 + 2] = (float)a.bg_b;
            continue;
        }
        double e1[3], e2[3], w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v0 = a.vertices[c[0] * 3 + k];
            e1[k] = a.vertices[c[1] * 3 + k] - v0;
            e2[k] = a.vertices[c[2] * 3 + k] - v0;
            w[k] = a.hit_points[p * 3 + k] - v0;
        }
        const double a11 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
        const double a12 = (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2];
        const double a22 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
        const double r1 = (w[0] * e1[0] + w[1] * e1[1]) + w[2] * e1[2];
        const double r2 = (w[0] * e2[0] + w[1] * e2[1]) + w[2] * e2[2];
        const double det = a11 * a22 - a12 * a12;
        double b1 = 0.0, b2 = 0.0;
        if (det > 0.0 && det < INFINITY) {
            b1 = (a22 * r1 - a12 * r2) / det;
            b2 = (a11 * r2 - a12 * r1) / det;
        }
        b1 = b1 > 0.0 ? b1 : 0.0;                                   // (NaN compares false)
        b2 = b2 > 0.0 ? b2 : 0.0;
        const double s = b1 + b2;
        if (s > 1.0) { b1 = b1 / s; b2 = b2 / s; }
        if (!(b1 <= 1.0)) b1 = 0.0;                                 // (inf / inf)
        if (!(b2 <= 1.0)) b2 = 0.0;
        const long cell = f >> 1;
        const double ox = (double)((cell % C) * n), oy = (double)((cell / C) * n);
        double x, y;
        if ((f & 1) == 0) { x = (ox + 0.5) + m * b1;              y = (oy + 0.5) + m * b2; }
        else              { x = (ox + ((double)n - 0.5)) - m * b1; y = (oy + ((double)n - 0.5)) - m * b2; }
        const double tx = x - 0.5, ty = y - 0.5, fx0 = floor(tx), fy0 = floor(ty);
        const double fx = tx - fx0, fy = ty - fy0;
        long x0 = (long)fx0, y0 = (long)fy0, x1 = x0 + 1, y1 = y0 + 1;
        x0 = x0 < 0 ? 0 : (x0 > S - 1 ? S - 1 : x0);
        x1 = x1 < 0 ? 0 : (x1 > S - 1 ? S - 1 : x1);
        y0 = y0 < 0 ? 0 : (y0 > S - 1 ? S - 1 : y0);
        y1 = y1 < 0 ? 0 : (y1 > S - 1 ? S - 1 : y1);
        const double w00 = (1.0 - fx) * (1.0 - fy), w10 = fx * (1.0 - fy), w01 = (1.0 - fx) * fy, w11 = fx * fy;
        const uint8_t* t00 = a.atlas + (y0 * S + x0) * 3;
        const uint8_t* t10 = a.atlas + (y0 * S + x1) * 3;
        const uint8_t* t01 = a.atlas + (y1 * S + x0) * 3;
        const uint8_t* t11 = a.atlas + (y1 * S + x1) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            a.rgb[p * 3 + k] = (float)(((w00 * (double)t00[k] + w10 * (double)t10[k]) + (w01 * (double)t01[k] + w11 * (double)t11[k])) / 255.0);
    }
}

}  // namespace vdn

// 256-thread blocks, grid-stride loops: enough blocks to cover n once, capped at a few waves of the 256 CUs
static inline unsigned tex_grid_of(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// the layout of an argument block: n >= 4 texels per cell edge, at least one cell, a cell half for every face
static int tex_layout_check(const VdnTexArgs* a) {
    if (a == nullptr || a->S < 4 || a->n < 4 || a->n > a->S || a->F < 0) return -1;
    if (a->F > INT_MAX || (int64_t)a->S * a->S > INT_MAX) return -10;
    const int64_t C = a->S / a->n, T = (int64_t)a->n * (a->n - 1) / 2;
    if ((a->F + 1) / 2 > C * C) return -1;
    if (a->F * T > INT_MAX) return -10;
    return 0;
}

static int tex_mesh_check(const VdnTexArgs* a) {
    if (a->vertices == nullptr || a->triangles == nullptr || a->error == nullptr || a->V < 1 || a->F < 1 ||
        (a->index_bytes != 4 && a->index_bytes != 8)) return -1;
    if (a->V > INT_MAX) return -10;
    return 0;
}

extern "C" int vdn_tex_points(const VdnTexArgs* a, void* stream) {
    int rc = tex_layout_check(a);
    if (rc == 0) rc = tex_mesh_check(a);
    if (rc != 0) return rc;
    if (a->points == nullptr || a->face == nullptr) return -1;
    const long P = (long)a->F * ((long)a->n * (a->n - 1) / 2);
    hipLaunchKernelGGL(vdn::tex_points_kernel, dim3(tex_grid_of(P)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_tex_gather(const VdnTexArgs* a, void* stream) {
    const int rc = tex_layout_check(a);
    if (rc != 0) return rc;
    if (a->atlas == nullptr || (a->F > 0 && a->colors == nullptr)) return -1;
    if (a->n_colors != a->F * ((int64_t)a->n * (a->n - 1) / 2)) return -1;
    hipLaunchKernelGGL(vdn::tex_gather_kernel, dim3(tex_grid_of((long)a->S * a->S)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_tex_sample(const VdnTexArgs* a, void* stream) {
    int rc = tex_layout_check(a);
    if (rc == 0) rc = tex_mesh_check(a);
    if (rc != 0) return rc;
    if (a->atlas == nullptr || a->hit_face == nullptr || a->hit_points == nullptr || a->rgb == nullptr || a->R < 1) return -1;
    if (a->R > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::tex_sample_kernel, dim3(tex_grid_of(a->R)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_tex_project(const VdnTexProjectArgs* a, void* stream) {
    if (a == nullptr || a->x == nullptr || a->x0 == nullptr || a->sdf == nullptr || a->g == nullptr || a->out == nullptr || a->N < 1 ||
        !(a->max_offset >= 0.0 && a->max_offset < INFINITY)) return -1;
    if (a->N > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::tex_project_kernel, dim3(tex_grid_of(a->N)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
