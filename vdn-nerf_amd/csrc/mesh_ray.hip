// Ray casting against a triangle mesh on a uniform grid (include/vdn_render.h: vdn_ray_bin_*, vdn_ray_cast, vdn_visibility_votes;
// vdn_hip/mesh.py: MeshGrid, visibility_votes). Built with -ffp-contract=off: every product and sum of the
// ray-triangle test is rounded on its own, so one (ray, triangle) pair gives one t whichever cell it is found through, and a numpy
// restatement in the same order gives the same bits. No LDS: one thread per triangle (binning) or per ray (casting); lanes of a
// wave walk different numbers of cells, so callers pass rays in a coherent order. The walk itself is k_ray_grid.h's (shared with
// mesh_photo.hip).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cmath>
#include "vdn_render.h"
#include "k_tri.h"
#include "k_project.h"
#include "k_ray_grid.h"

namespace vdn {

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
        const RayHit hit = a.any_hit != 0 ? cast_ray<true>(g, o, d, a.t_min, a.t_max, skip, -1) : cast_ray<false>(g, o, d, a.t_min, a.t_max, skip, -1);
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
            if (cast_ray<true>(g, o, d, 0.0, 1.0 - a.eps, v, -1).face < 0) atomicAdd(a.n_visible + v, 1);
        }
    }
}

}  // namespace vdn

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
