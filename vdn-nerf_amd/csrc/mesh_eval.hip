// Mesh evaluation on the device (include/vdn_render.h: vdn_surf_*, vdn_nn_*, vdn_thin_round): area-weighted surface sampling of a
// triangle mesh, exact nearest neighbours on a uniform grid - the two halves of an accuracy / completeness / Chamfer figure against a
// scanned point cloud (vdn_train/mesh_eval.py) - and greedy radius thinning of a cloud on the same grid. Gather-bound integer / float
// work, no LDS: one thread per triangle, per sample, per point or per query. The prefix sum, the stable sorts and the cell-start
// table between the passes are the caller's torch ops. The grid search itself is in k_nn.h, shared with mesh_align.hip.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include "vdn_render.h"
#include "k_tri.h"
#include "k_nn.h"

namespace vdn {

// ---- surface sampling -----------------------------------------------------------------------------------------------------------
__device__ inline bool surf_corners(const VdnSurfArgs& a, long f, long* i) {
    return tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i);      // (k_tri.h, shared with mesh_clean.hip)
}

__global__ void surf_count_kernel(VdnSurfArgs a) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= (long)a.F) return;
    long i[3];
    int n = 0;
    if (!surf_corners(a, f, i)) {
        *a.error = 1;                  // (every writer stores the same word)
    } else {
        const double area = tri_area(a.vertices, i);
        const double r = area / (a.spacing * a.spacing);
        if (area > 0.0 && r < INFINITY) n = r >= (double)INT_MAX ? INT_MAX : (int)ceil(r);      // (NaN fails `area > 0`)
    }
    a.counts[f] = n;
}

__global__ void surf_emit_kernel(VdnSurfArgs a) {
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (long)a.S) return;
    // the last triangle whose exclusive offset is <= s: the triangles behind it that share the offset have no samples
    long lo = 0, hi = (long)a.F;                     // invariant: offsets[lo] <= s, offsets[hi] > s (offsets[F] = S)
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (a.offsets[mid] <= s) lo = mid; else hi = mid;
    }
    const long f = lo;
    long i[3];
    if (!surf_corners(a, f, i)) return;              // (such a triangle has no samples: unreachable, and nothing is read out of bounds)
    const double j1 = (double)(s - a.offsets[f] + 1);
    double u = 0.5 + j1 * 0.7548776662466927, v = 0.5 + j1 * 0.5698402909980532;
    u -= floor(u);
    v -= floor(v);
    if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double pa = (double)a.vertices[i[0] * 3 + d], pb = (double)a.vertices[i[1] * 3 + d], pc = (double)a.vertices[i[2] * 3 + d];
        a.points[s * 3 + d] = (float)(pa + u * (pb - pa) + v * (pc - pa));
    }
    a.face[s] = (int)f;
}

// ---- nearest neighbour on a uniform grid ------------------------------------------------------------------------------------------
__global__ void nn_bin_kernel(VdnNnArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)a.N) return;
    const int cx = nn_axis(a.pts[i * 3 + 0], a.lo_x, a.h, a.nx), cy = nn_axis(a.pts[i * 3 + 1], a.lo_y, a.h, a.ny),
              cz = nn_axis(a.pts[i * 3 + 2], a.lo_z, a.h, a.nz);
    a.cell[i] = (cz * a.ny + cy) * a.nx + cx;
}

__global__ void nn_query_kernel(VdnNnArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)a.N) return;
    const long q = a.order != nullptr ? (long)a.order[t] : t;
    const float qx = a.pts[q * 3 + 0], qy = a.pts[q * 3 + 1], qz = a.pts[q * 3 + 2];
    NnBest b;
    const int k = nn_search(a, qx, qy, qz, b);           // (k_nn.h, shared with mesh_align.hip)
    float d;
    const bool hit = nn_hit(b, a.max_dist, &d);
    a.dist[q] = hit ? d : INFINITY;
    a.idx[q] = hit ? (int64_t)b.idx : (int64_t)-1;
    if (a.rings != nullptr) a.rings[q] = k + 1;
}

// ---- greedy radius thinning: one round -----------------------------------------------------------------------------------------
enum { kThinUndecided = 0, kThinKept = 1, kThinRemoved = 2 };

// the state of record t after looking at every lower-index point within the radius, as far as those are decided themselves
__device__ inline int thin_decide(const VdnThinArgs& a, int t) {
    const float4* rec = (const float4*)a.rec;
    const float4 me = rec[t];
    const int my_id = __float_as_int(me.w);
    // the record's own cell: vdn_nn_bin's expression on the same fp32 bits, so the cell it was sorted into
    const int cx = nn_axis(me.x, a.lo_x, a.h, a.nx), cy = nn_axis(me.y, a.lo_y, a.h, a.ny), cz = nn_axis(me.z, a.lo_z, a.h, a.nz);
    const float r2 = a.radius * a.radius;
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, a.nx - 1);
    bool waiting = false;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, a.nz - 1); ++z) {
        for (int y = max(cy - 1, 0); y <= min(cy + 1, a.ny - 1); ++y) {
            const int row = (z * a.ny + y) * a.nx;
            // the three x-cells of a row are one contiguous record range (nn_scan's trick)
            const int begin = max(a.cell_start[row + x0], 0), end = min(a.cell_start[row + x1 + 1], (int)a.N);
            for (int r = begin; r < end; ++r) {
                const float4 p = rec[r];
                if (__float_as_int(p.w) >= my_id) continue;          // (also the record itself)
                const float dx = me.x - p.x, dy = me.y - p.y, dz = me.z - p.z;
                if (!(dx * dx + dy * dy + dz * dz <= r2)) continue;
                // another lane may be storing this word right now: any of its values is a valid, final-or-undecided state
                const int s = __hip_atomic_load(&a.state[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (s == kThinKept) return kThinRemoved;
                waiting |= s == kThinUndecided;
            }
        }
    }
    return waiting ? kThinUndecided : kThinKept;
}

__global__ void thin_round_kernel(VdnThinArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool undecided = false;
    if (t < (long)a.N && __hip_atomic_load(&a.state[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kThinUndecided) {
        const int s = thin_decide(a, (int)t);
        if (s != kThinUndecided) __hip_atomic_store(&a.state[t], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        undecided = s == kThinUndecided;
    }
    // every lane of the wave is here again (no early return above): one add per wave that has something to add
    const unsigned long long left = __ballot(undecided);
    if ((threadIdx.x & 63) == 0 && left != 0) atomicAdd(a.undecided, (int)__popcll(left));
}

}  // namespace vdn

static inline unsigned grid_of(long n) { return (unsigned)((n + 255) / 256); }

extern "C" int vdn_surf_count(const VdnSurfArgs* a, void* stream) {
    if (a == nullptr || a->triangles == nullptr || a->counts == nullptr || a->error == nullptr || a->F < 1 || a->V < 0 ||
        (a->V > 0 && a->vertices == nullptr) || (a->index_bytes != 4 && a->index_bytes != 8) || !(a->spacing > 0.0)) return -1;
    if (a->F > INT_MAX || a->V > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::surf_count_kernel, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_surf_emit(const VdnSurfArgs* a, void* stream) {
    if (a == nullptr || a->triangles == nullptr || a->vertices == nullptr || a->offsets == nullptr || a->points == nullptr ||
        a->face == nullptr || a->F < 1 || a->V < 1 || a->S < 1 || (a->index_bytes != 4 && a->index_bytes != 8)) return -1;
    if (a->F > INT_MAX || a->V > INT_MAX || a->S > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::surf_emit_kernel, dim3(grid_of(a->S)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

static int nn_grid_check(const VdnNnArgs* a) {
    if (a == nullptr || a->pts == nullptr || a->N < 1 || a->nx < 1 || a->ny < 1 || a->nz < 1 || !(a->h > 0.0f) || !(a->h < INFINITY)) return -1;
    if (a->N > INT_MAX || (int64_t)a->nx * a->ny * a->nz >= (int64_t)INT_MAX) return -10;
    return 0;
}

extern "C" int vdn_nn_bin(const VdnNnArgs* a, void* stream) {
    const int rc = nn_grid_check(a);
    if (rc != 0) return rc;
    if (a->cell == nullptr) return -1;
    hipLaunchKernelGGL(vdn::nn_bin_kernel, dim3(grid_of(a->N)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_nn_query(const VdnNnArgs* a, void* stream) {
    const int rc = nn_grid_check(a);
    if (rc != 0) return rc;
    if (a->ref == nullptr || a->cell_start == nullptr || a->dist == nullptr || a->idx == nullptr || a->R < 1 || !(a->margin >= 0.0f) ||
        !(a->max_dist >= 0.0f)) return -1;
    if (a->R > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::nn_query_kernel, dim3(grid_of(a->N)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_thin_round(const VdnThinArgs* a, void* stream) {
    if (a == nullptr || a->rec == nullptr || a->cell_start == nullptr || a->state == nullptr || a->undecided == nullptr || a->N < 1 ||
        a->nx < 1 || a->ny < 1 || a->nz < 1 || !(a->h > 0.0f) || !(a->h < INFINITY) || !(a->radius > 0.0f) || !(a->radius < INFINITY)) return -1;
    if (a->N > INT_MAX || (int64_t)a->nx * a->ny * a->nz >= (int64_t)INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::thin_round_kernel, dim3(grid_of(a->N)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
