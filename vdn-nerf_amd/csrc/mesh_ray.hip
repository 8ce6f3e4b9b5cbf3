// Ray casting against a triangle mesh on a uniform grid (include/vdn_render.h: vdn_ray_bin_*, vdn_ray_cast, vdn_visibility_votes;
// vdn_hip/mesh.py: MeshGrid, visibility_votes). Built with -ffp-contract=off: every product and sum of the
// ray-triangle test is rounded on its own, so one (ray, triangle) pair gives one t whichever cell it is found through, and a numpy
// restatement in the same order gives the same bits. No LDS: one thread per triangle (binning) or per ray (casting); lanes of a
// wave walk different numbers of cells, so callers pass rays in a coherent order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cmath>
#include "vdn_render.h"
#include "k_tri.h"
#include "k_project.h"

namespace vdn {

struct RayGrid {
    const float* records;
    const int32_t* cell_start;
    const int32_t* refs;
    long F, n_refs;
    double lo[3], h, margin;
    int n[3];
};

template <class A>
__device__ inline RayGrid ray_grid(const A& a) {
    RayGrid g;
    g.records = a.records, g.cell_start = a.cell_start, g.refs = a.refs, g.F = (long)a.F, g.n_refs = (long)a.n_refs;
    g.lo[0] = a.lo_x, g.lo[1] = a.lo_y, g.lo[2] = a.lo_z, g.h = a.h, g.margin = a.margin;
    g.n[0] = a.nx, g.n[1] = a.ny, g.n[2] = a.nz;
    return g;
}

// cell coordinate of x on one axis, clamped into the grid (NaN lands in cell 0: the comparisons are made in double)
__device__ inline int cell_coord(double x, double lo, double h, int n) {
    return (int)fmin(fmax(floor((x - lo) / h), 0.0), (double)(n - 1));
}

// ---- binning ------------------------------------------------------------------------------------------------------------------------
// 0: referenced, with its corners p and the cell range [c0, c1] of its grown box; 1: not referenced; 2: a corner index out of range
__device__ inline int tri_cells(const VdnRayGridArgs& a, long f, long* i, float p[3][3], int* c0, int* c1) {
    if (!tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i)) return 2;
    if (i[0] == i[1] || i[1] == i[2] || i[0] == i[2]) return 1;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[c][k] = a.vertices[i[c] * 3 + k];
            if (!(fabsf(p[c][k]) < INFINITY)) return 1;
        }
    const double area = tri_area(a.vertices, i);
    if (!(area > 0.0 && area < INFINITY)) return 1;
    const double lo[3] = {a.lo_x, a.lo_y, a.lo_z};
    const int n[3] = {a.nx, a.ny, a.nz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mn = (double)fminf(p[0][k], fminf(p[1][k], p[2][k])), mx = (double)fmaxf(p[0][k], fmaxf(p[1][k], p[2][k]));
        c0[k] = cell_coord(mn - a.margin, lo[k], a.h, n[k]);
        c1[k] = cell_coord(mx + a.margin, lo[k], a.h, n[k]);
    }
    return 0;
}

template <bool FILL>
__global__ void __launch_bounds__(256) ray_bin_kernel(VdnRayGridArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < (long)a.F; f += stride) {
        long i[3];
        float p[3][3];
        int c0[3], c1[3];
        const int kind = tri_cells(a, f, i, p, c0, c1);
        if (!FILL) {
            float4* rec = (float4*)a.records + f * 3;
            if (kind == 0) {
                rec[0] = make_float4(p[0][0], p[0][1], p[0][2], p[1][0]);
                rec[1] = make_float4(p[1][1], p[1][2], p[2][0], p[2][1]);
                rec[2] = make_float4(p[2][2], __int_as_float((int)i[0]), __int_as_float((int)i[1]), __int_as_float((int)i[2]));
            } else {
                rec[0] = rec[1] = rec[2] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kind == 2) *a.error = 1;                   // (every writer stores the same word)
            }
        }
        if (kind != 0) continue;
        for (int z = c0[2]; z <= c1[2]; ++z)
            for (int y = c0[1]; y <= c1[1]; ++y)
                for (int x = c0[0]; x <= c1[0]; ++x) {
                    const long c = ((long)z * a.ny + y) * a.nx + x;
                    if (!FILL) {
                        atomicAdd(a.cell_count + c, 1);
                    } else {
                        const long slot = (long)atomicAdd(a.cursor + c, 1);
                        if (slot >= 0 && slot < (long)a.n_refs) a.refs[slot] = (int32_t)f;
                    }
                }
    }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------
struct RayHit {
    double t;
    int face, tests;
};

// o + t d against the grid's triangles, t_min < t < t_max; skip: a vertex index whose triangles are ignored, or -1
template <bool ANY>
__device__ inline RayHit cast_ray(const RayGrid& g, const double* o, const double* d, double t_min, double t_max, long skip) {
    RayHit hit;
    hit.t = INFINITY, hit.face = -1, hit.tests = 0;
    // misses decided before the loop: a ray that is not finite, an empty or NaN window, no direction, no overlap with the box
    if (!(t_min < t_max)) return hit;
    double inv[3], t0 = t_min, t1 = t_max;
    bool moving[3], any = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(fabs(o[k]) < INFINITY && fabs(d[k]) < INFINITY)) return hit;
        inv[k] = 1.0 / d[k];
        moving[k] = d[k] != 0.0 && fabs(inv[k]) < INFINITY;      // (a component too small for a finite reciprocal counts as zero)
        any = any || moving[k];
    }
    if (!any) return hit;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double b0 = g.lo[k] - g.margin, b1 = g.lo[k] + (double)g.n[k] * g.h + g.margin;
        if (moving[k]) {
            const double ta = (b0 - o[k]) * inv[k], tb = (b1 - o[k]) * inv[k];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        } else if (!(o[k] >= b0 && o[k] <= b1)) {
            return hit;
        }
    }
    if (!(t0 <= t1)) return hit;
    int i[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) i[k] = cell_coord(o[k] + t0 * d[k], g.lo[k], g.h, g.n[k]);

    const float4* records = (const float4*)g.records;
    const int max_steps = g.n[0] + g.n[1] + g.n[2] + 3;
    for (int step = 0; step < max_steps; ++step) {
        const long c = ((long)i[2] * g.n[1] + i[1]) * g.n[0] + i[0];
        const long kb = max((long)g.cell_start[c], 0L), ke = min((long)g.cell_start[c + 1], g.n_refs);
        for (long k = kb; k < ke; ++k) {
            const long f = (long)g.refs[k];
            if (f < 0 || f >= g.F) continue;
            const float4 r0 = records[f * 3], r1 = records[f * 3 + 1], r2 = records[f * 3 + 2];
            if (skip >= 0 && ((long)__float_as_int(r2.y) == skip || (long)__float_as_int(r2.z) == skip || (long)__float_as_int(r2.w) == skip))
                continue;
            ++hit.tests;
            const double ax = (double)r0.x, ay = (double)r0.y, az = (double)r0.z;
            const double e1x = (double)r0.w - ax, e1y = (double)r1.x - ay, e1z = (double)r1.y - az;
            const double e2x = (double)r1.z - ax, e2y = (double)r1.w - ay, e2z = (double)r2.x - az;
            const double px = d[1] * e2z - d[2] * e2y, py = d[2] * e2x - d[0] * e2z, pz = d[0] * e2y - d[1] * e2x;
            const double det = e1x * px + e1y * py + e1z * pz;
            if (det == 0.0 || !(fabs(det) < INFINITY)) continue;
            const double idet = 1.0 / det;
            const double sx = o[0] - ax, sy = o[1] - ay, sz = o[2] - az;
            const double u = (sx * px + sy * py + sz * pz) * idet;
            const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
            const double v = (d[0] * qx + d[1] * qy + d[2] * qz) * idet;
            const double t = (e2x * qx + e2y * qy + e2z * qz) * idet;
            if (!(u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t > t_min && t < t_max)) continue;
            if (t < hit.t || (t == hit.t && (int)f < hit.face)) hit.t = t, hit.face = (int)f;
            if (ANY) return hit;
        }
        // the parameter at which the ray leaves this cell, from the cell index (nothing accumulates over the walk)
        double t_exit = INFINITY;
        int axis = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!moving[k]) continue;                             // never crossed
            const double plane = g.lo[k] + (double)(i[k] + (d[k] > 0.0 ? 1 : 0)) * g.h;
            const double tn = (plane - o[k]) * inv[k];
            if (tn < t_exit) t_exit = tn, axis = k;               // (the lower axis on equal parameters)
        }
        if (hit.t <= t_exit) break;
        if (!(t_exit < t1)) break;
        bool outside = false;
#pragma unroll
        for (int k = 0; k < 3; ++k)                               // (selects, not a runtime index: the arrays stay in registers)
            if (k == axis) {
                i[k] += d[k] > 0.0 ? 1 : -1;
                outside = i[k] < 0 || i[k] >= g.n[k];
            }
        if (outside) break;
    }
    return hit;
}

__global__ void __launch_bounds__(256) ray_cast_kernel(VdnRayCastArgs a) {
    const RayGrid g = ray_grid(a);
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < (long)a.R; r += stride) {
        const double o[3] = {a.origins[r * 3], a.origins[r * 3 + 1], a.origins[r * 3 + 2]};
        const double d[3] = {a.directions[r * 3], a.directions[r * 3 + 1], a.directions[r * 3 + 2]};
        long skip = -1;
        if (a.skip_vertex != nullptr) {
            skip = (long)a.skip_vertex[r];
            if (skip < 0 || skip > INT_MAX) skip = -1;             // (no corner index of a record is outside [0, 2^31))
        }
        const RayHit hit = a.any_hit != 0 ? cast_ray<true>(g, o, d, a.t_min, a.t_max, skip) : cast_ray<false>(g, o, d, a.t_min, a.t_max, skip);
        a.t[r] = hit.t;
        a.face[r] = (int64_t)hit.face;
        if (a.tests != nullptr) a.tests[r] = hit.tests;
    }
}

// camera-major: blockIdx.y strides over the cameras, so the lanes of a wave share the origin and neighbouring vertices
__global__ void __launch_bounds__(256) visibility_votes_kernel(VdnVisibilityArgs a) {
    const RayGrid g = ray_grid(a);
    const long stride = (long)gridDim.x * blockDim.x;
    for (long n = blockIdx.y; n < (long)a.N; n += gridDim.y) {
        const double o[3] = {a.centres[n * 3], a.centres[n * 3 + 1], a.centres[n * 3 + 2]};
        for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < (long)a.V; v += stride) {
            const double x = (double)a.vertices[v * 3 + 0], y = (double)a.vertices[v * 3 + 1], z = (double)a.vertices[v * 3 + 2];
            long px, py;
            if (!project_in_image(a.P + n * 12, x, y, z, a.H, a.W, &px, &py)) continue;
            atomicAdd(a.n_in_image + v, 1);
            const double d[3] = {x - o[0], y - o[1], z - o[2]};
            if (cast_ray<true>(g, o, d, 0.0, 1.0 - a.eps, v).face < 0) atomicAdd(a.n_visible + v, 1);
        }
    }
}

}  // namespace vdn

static inline unsigned grid_of(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// nx * ny * nz as a 32-bit count (with room for the cell_start table's last entry), or -1
static long cell_total(int32_t nx, int32_t ny, int32_t nz) {
    const int64_t xy = (int64_t)nx * ny;
    if (xy >= INT_MAX || xy * nz >= INT_MAX) return -1;
    return (long)(xy * nz);
}

static inline bool geometry_ok(int32_t nx, int32_t ny, int32_t nz, double lo_x, double lo_y, double lo_z, double h, double margin) {
    return nx >= 1 && ny >= 1 && nz >= 1 && std::isfinite(lo_x) && std::isfinite(lo_y) && std::isfinite(lo_z) && std::isfinite(h) && h > 0.0 &&
           std::isfinite(margin) && margin >= 0.0;
}

static int bin_check(const VdnRayGridArgs* a) {
    if (a == nullptr || a->vertices == nullptr || a->triangles == nullptr || a->F < 1 || a->V < 1 || (a->index_bytes != 4 && a->index_bytes != 8) ||
        !geometry_ok(a->nx, a->ny, a->nz, a->lo_x, a->lo_y, a->lo_z, a->h, a->margin)) return -1;
    if (a->V > INT_MAX || a->F > INT_MAX || cell_total(a->nx, a->ny, a->nz) < 0) return -10;
    return 0;
}

extern "C" int vdn_ray_bin_count(const VdnRayGridArgs* a, void* stream) {
    const int rc = bin_check(a);
    if (rc != 0) return rc;
    if (a->cell_count == nullptr || a->records == nullptr || a->error == nullptr) return -1;
    hipLaunchKernelGGL(vdn::ray_bin_kernel<false>, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_ray_bin_fill(const VdnRayGridArgs* a, void* stream) {
    const int rc = bin_check(a);
    if (rc != 0) return rc;
    if (a->cursor == nullptr || a->refs == nullptr || a->n_refs < 1) return -1;
    if (a->n_refs > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::ray_bin_kernel<true>, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_ray_cast(const VdnRayCastArgs* a, void* stream) {
    if (a == nullptr || a->origins == nullptr || a->directions == nullptr || a->records == nullptr || a->cell_start == nullptr || a->refs == nullptr ||
        a->t == nullptr || a->face == nullptr || a->R < 1 || a->F < 0 || a->n_refs < 0 ||
        !geometry_ok(a->nx, a->ny, a->nz, a->lo_x, a->lo_y, a->lo_z, a->h, a->margin)) return -1;
    if (a->R > INT_MAX || a->F > INT_MAX || a->n_refs > INT_MAX || cell_total(a->nx, a->ny, a->nz) < 0) return -10;
    hipLaunchKernelGGL(vdn::ray_cast_kernel, dim3(grid_of(a->R)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_visibility_votes(const VdnVisibilityArgs* a, void* stream) {
    if (a == nullptr || a->vertices == nullptr || a->P == nullptr || a->centres == nullptr || a->records == nullptr || a->cell_start == nullptr ||
        a->refs == nullptr || a->n_in_image == nullptr || a->n_visible == nullptr || a->V < 1 || a->N < 1 || a->F < 0 || a->n_refs < 0 ||
        a->H < 1 || a->W < 1 || !(a->eps >= 0.0 && a->eps < 1.0) ||
        !geometry_ok(a->nx, a->ny, a->nz, a->lo_x, a->lo_y, a->lo_z, a->h, a->margin)) return -1;
    if (a->V > INT_MAX || a->N > INT_MAX || a->F > INT_MAX || a->n_refs > INT_MAX || cell_total(a->nx, a->ny, a->nz) < 0) return -10;
    const unsigned gy = (unsigned)(a->N < 65535 ? a->N : 65535);
    hipLaunchKernelGGL(vdn::visibility_votes_kernel, dim3(grid_of(a->V), gy), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
