// The uniform grid over a mesh's triangles and the walk of one ray through it, shared by the ray-casting kernels (mesh_ray.hip) and
// the photo projection of the texture bake (mesh_photo.hip): one device function, so that a segment is occluded for the one exactly
// when it is for the other. Both files are built with -ffp-contract=off: every product and sum of the ray-triangle test is rounded on
// its own (include/vdn_render.h, vdn_ray_cast, has the rules).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cmath>

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

// ---- the walk -----------------------------------------------------------------------------------------------------------------------
struct RayHit {
    double t;
    int face, tests;
};

// o + t d against the grid's triangles, t_min < t < t_max; skip: a vertex index whose triangles are ignored, or -1; skip_face: a face
// index that is ignored, or -1
template <bool ANY>
__device__ inline RayHit cast_ray(const RayGrid& g, const double* o, const double* d, double t_min, double t_max, long skip, long skip_face) {
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
            if (f < 0 || f >= g.F || f == skip_face) continue;
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

}  // namespace vdn

// ---- the host's checks of an argument block's grid fields ----------------------------------------------------------------------------
static inline unsigned grid_of(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// nx * ny * nz as a 32-bit count (with room for the cell_start table's last entry), or -1
static inline long cell_total(int32_t nx, int32_t ny, int32_t nz) {
    const int64_t xy = (int64_t)nx * ny;
    if (xy >= INT_MAX || xy * nz >= INT_MAX) return -1;
    return (long)(xy * nz);
}

static inline bool geometry_ok(int32_t nx, int32_t ny, int32_t nz, double lo_x, double lo_y, double lo_z, double h, double margin) {
    return nx >= 1 && ny >= 1 && nz >= 1 && std::isfinite(lo_x) && std::isfinite(lo_y) && std::isfinite(lo_z) && std::isfinite(h) && h > 0.0 &&
           std::isfinite(margin) && margin >= 0.0;
}
