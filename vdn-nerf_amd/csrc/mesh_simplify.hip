// Mesh simplification on the device (include/vdn_render.h: vdn_simplify_*, vdn_segment_mean, vdn_cluster_*, vdn_octree_*): vertex clustering on a
// uniform grid with quadric error placement (vdn_hip/mesh.py: cluster_quadrics, simplify_mesh). A mark pass and a key
// pass per triangle / vertex, the corner records per triangle, then two segmented sums - a wave per cluster, lanes striding the
// cluster's list, a fixed-order tree across the lanes - and one thread per cluster for the 3 x 3 solve. All arithmetic is double on
// the widened fp32 vertices; the file is built with -ffp-contract=off, so every product and sum rounds on its own and a numpy model
// can follow the sums to the bit. No float atomics, no LDS. The octree levels of the adaptive mode follow below the
// placement they share: a thread per node merges its children's records, a thread per node decides, a thread per finest cluster climbs.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include "vdn_render.h"
#include "k_tri.h"

namespace vdn {

__device__ inline bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

__global__ void simplify_mark_kernel(VdnSimplifyArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < (long)a.F; f += stride) {
        long i[3];
        bool live = false;
        if (!tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i)) *a.error = 1;      // (every writer stores the same word)
        else live = finite3(a.vertices + i[0] * 3) && finite3(a.vertices + i[1] * 3) && finite3(a.vertices + i[2] * 3);
        a.live[f] = live ? 1 : 0;
        if (live) a.vertex_used[i[0]] = a.vertex_used[i[1]] = a.vertex_used[i[2]] = 1;     // (plain stores of one value: order-free)
    }
}

// cell index of one coordinate relative to the grid's first cell, or -1 outside [0, n) (NaN and inf fail the comparisons)
__device__ inline long cell_of(float p, double origin, double h, long lo, long n) {
    const double c = floor(((double)p - origin) / h) - (double)lo;
    return (c >= 0.0 && c < (double)n) ? (long)c : -1;
}

__global__ void simplify_keys_kernel(VdnSimplifyArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < (long)a.V; v += stride) {
        const long ix = cell_of(a.vertices[v * 3 + 0], a.origin_x, a.h, (long)a.lo_x, (long)a.nx);
        const long iy = cell_of(a.vertices[v * 3 + 1], a.origin_y, a.h, (long)a.lo_y, (long)a.ny);
        const long iz = cell_of(a.vertices[v * 3 + 2], a.origin_z, a.h, (long)a.lo_z, (long)a.nz);
        a.key[v] = (ix < 0 || iy < 0 || iz < 0) ? -1 : ix + (long)a.nx * (iy + (long)a.ny * iz);
    }
}

__global__ void simplify_records_kernel(VdnSimplifyArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long C = (long)a.C;
    for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < (long)a.F; f += stride) {
        long i[3], c[3] = {C, C, C};
        bool live = a.live[f] != 0 && tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i);
        if (live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c[k] = (long)a.vertex_cluster[i[k]];
                if (c[k] < 0 || c[k] >= C) live = false;          // (a live triangle's corners are all clustered: never taken)
            }
            if (!live) c[0] = c[1] = c[2] = C;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.corner_cluster[f * 3 + k] = c[k];
        const bool survive = live && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
        a.survive[f] = survive ? 1 : 0;
        long r[3] = {C, C, C};
        if (survive) {
            const int s = (c[0] < c[1] && c[0] < c[2]) ? 0 : (c[1] < c[2] ? 1 : 2);      // the smallest id first, same cyclic order
            r[0] = c[s]; r[1] = c[(s + 1) % 3]; r[2] = c[(s + 2) % 3];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.canonical[f * 3 + k] = r[k];
    }
}

// partial[l] += partial[l + s] for s = 32 .. 1: lane 0 ends with the sum in the documented order (the lanes l >= s add values nobody
// reads afterwards)
__device__ inline double wave_tree(double x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s, 64);
    return x;
}

// one wave per segment; 256-thread blocks hold four of them
__global__ void segment_mean_kernel(VdnSegmentMeanArgs a) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * (blockDim.x >> 6);
    for (long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); s < (long)a.C; s += waves) {
        long b = (long)a.start[s], e = (long)a.start[s + 1];
        if (b < 0) b = 0;
        if (e > (long)a.M) e = (long)a.M;
        const double count = (double)(e > b ? e - b : 0);
        for (int k = 0; k < a.K; ++k) {
            double acc = 0.0;
            for (long j = b + lane; j < e; j += 64) {
                const long r = (long)a.members[j];
                if (r >= 0 && r < (long)a.N) acc += (double)a.rows[r * a.K + k];
            }
            acc = wave_tree(acc);
            if (lane == 0) a.out[s * a.K + k] = acc / count;
        }
    }
}

__global__ void cluster_quadrics_kernel(VdnClusterQuadricArgs a) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * (blockDim.x >> 6);
    for (long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); s < (long)a.C; s += waves) {
        long b = (long)a.start[s], e = (long)a.start[s + 1];
        if (b < 0) b = 0;
        if (e > (long)a.M) e = (long)a.M;
        const double cx = a.centre[s * 3 + 0], cy = a.centre[s * 3 + 1], cz = a.centre[s * 3 + 2];
        double q[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) q[k] = 0.0;
        for (long j = b + lane; j < e; j += 64) {
            const long rec = (long)a.members[j];
            long i[3];
            if (rec < 0 || rec / 3 >= (long)a.F || !tri_corners(a.triangles, a.index_bytes, (long)a.V, rec / 3, i)) continue;
            double p[3][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                p[c][0] = (double)a.vertices[i[c] * 3 + 0] - cx;
                p[c][1] = (double)a.vertices[i[c] * 3 + 1] - cy;
                p[c][2] = (double)a.vertices[i[c] * 3 + 2] - cz;
            }
            const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const double w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const double n0 = u[1] * w[2] - u[2] * w[1], n1 = u[2] * w[0] - u[0] * w[2], n2 = u[0] * w[1] - u[1] * w[0];
            const double d = -((n0 * p[0][0] + n1 * p[0][1]) + n2 * p[0][2]);
            q[0] += n0 * n0; q[1] += n0 * n1; q[2] += n0 * n2; q[3] += n1 * n1; q[4] += n1 * n2; q[5] += n2 * n2;
            q[6] += n0 * d;  q[7] += n1 * d;  q[8] += n2 * d;  q[9] += d * d;
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const double t = wave_tree(q[k]);
            if (lane == 0) a.quadric[s * 10 + k] = t;
        }
    }
}

// the placement of vdn_cluster_place and of every octree level (include/vdn_render.h): x relative to the cell centre -> status
__device__ inline int place_quadric(const double* q, const double* m, double h, double eps, double* x) {
    x[0] = m[0]; x[1] = m[1]; x[2] = m[2];
    const double tr = (q[0] + q[3]) + q[5];
    if (!(tr > 0.0 && tr < INFINITY)) return 1;
    const double r = eps * tr;
    const double A00 = q[0] + r, A01 = q[1], A02 = q[2], A11 = q[3] + r, A12 = q[4], A22 = q[5] + r;
    const double g0 = -q[6] - ((q[0] * m[0] + q[1] * m[1]) + q[2] * m[2]);
    const double g1 = -q[7] - ((q[1] * m[0] + q[3] * m[1]) + q[4] * m[2]);
    const double g2 = -q[8] - ((q[2] * m[0] + q[4] * m[1]) + q[5] * m[2]);
    // the inverse of the symmetric matrix by cofactors
    const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
    const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
    const double det = (A00 * c00 + A01 * c01) + A02 * c02;
    const double y[3] = {m[0] + ((c00 * g0 + c01 * g1) + c02 * g2) / det, m[1] + ((c01 * g0 + c11 * g1) + c12 * g2) / det,
                         m[2] + ((c02 * g0 + c12 * g1) + c22 * g2) / det};
    const double half = 0.5 * h;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && fabs(y[k]) <= half;          // (NaN fails the comparison)
    if (!ok) return 2;
    x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
    return 0;
}

__global__ void cluster_place_kernel(VdnClusterQuadricArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < (long)a.C; s += stride) {
        const double m[3] = {a.mean[s * 3 + 0], a.mean[s * 3 + 1], a.mean[s * 3 + 2]};
        double x[3];
        const int status = place_quadric(a.quadric + s * 10, m, a.h, a.eps, x);
#pragma unroll
        for (int k = 0; k < 3; ++k) a.position[s * 3 + k] = a.centre[s * 3 + k] + x[k];
        a.status[s] = (uint8_t)status;
    }
}

// ---- octree levels (include/vdn_render.h: vdn_octree_*) ----------------------------------------------------------------
// the index of `key` in the ascending keys[0 .. n), or -1
__device__ inline long find_key(const int64_t* keys, long n, long key) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if ((long)keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && (long)keys[lo] == key) ? lo : -1;
}

__global__ void octree_merge_kernel(VdnOctreeMergeArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < (long)a.C; p += stride) {
        double q[10], m[3];
        if (a.children != nullptr) {
            double S[3] = {0.0, 0.0, 0.0};
            long n = 0;
#pragma unroll
            for (int k = 0; k < 10; ++k) q[k] = 0.0;
            const long i[3] = {(long)a.cell[p * 3 + 0], (long)a.cell[p * 3 + 1], (long)a.cell[p * 3 + 2]};
            const double quarter = 0.25 * a.h;
            for (int s = 0; s < 8; ++s) {
                const int bit[3] = {s & 1, (s >> 1) & 1, (s >> 2) & 1};
                const long rx = 2 * i[0] + bit[0] - (long)a.lo_x, ry = 2 * i[1] + bit[1] - (long)a.lo_y, rz = 2 * i[2] + bit[2] - (long)a.lo_z;
                long c = -1;
                if (rx >= 0 && rx < (long)a.nx && ry >= 0 && ry < (long)a.ny && rz >= 0 && rz < (long)a.nz)
                    c = find_key(a.child_key, (long)a.Cc, rx + (long)a.nx * (ry + (long)a.ny * rz));
                a.children[p * 8 + s] = c;
                if (c < 0) continue;
                const double* cq = a.child_quadric + c * 10;
                const double* cm = a.child_mean + c * 3;
                const double d[3] = {bit[0] ? quarter : -quarter, bit[1] ? quarter : -quarter, bit[2] ? quarter : -quarter};
                const double Ad0 = (cq[0] * d[0] + cq[1] * d[1]) + cq[2] * d[2];
                const double Ad1 = (cq[1] * d[0] + cq[3] * d[1]) + cq[4] * d[2];
                const double Ad2 = (cq[2] * d[0] + cq[4] * d[1]) + cq[5] * d[2];
#pragma unroll
                for (int k = 0; k < 6; ++k) q[k] += cq[k];
                q[6] += cq[6] - Ad0; q[7] += cq[7] - Ad1; q[8] += cq[8] - Ad2;
                q[9] += (cq[9] - 2.0 * ((cq[6] * d[0] + cq[7] * d[1]) + cq[8] * d[2])) + ((d[0] * Ad0 + d[1] * Ad1) + d[2] * Ad2);
                const long nc = (long)a.child_count[c];
                n += nc;
#pragma unroll
                for (int k = 0; k < 3; ++k) S[k] += (double)nc * (cm[k] + d[k]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = S[k] / (double)n;
#pragma unroll
            for (int k = 0; k < 10; ++k) a.quadric[p * 10 + k] = q[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) a.mean[p * 3 + k] = m[k];
            a.count[p] = n;
        } else {
#pragma unroll
            for (int k = 0; k < 10; ++k) q[k] = a.quadric[p * 10 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = a.mean[p * 3 + k];
        }
        double x[3];
        const int status = place_quadric(q, m, a.h, a.eps, x);
        const double Ax0 = (q[0] * x[0] + q[1] * x[1]) + q[2] * x[2];
        const double Ax1 = (q[1] * x[0] + q[3] * x[1]) + q[4] * x[2];
        const double Ax2 = (q[2] * x[0] + q[4] * x[1]) + q[5] * x[2];
        const double e = (((x[0] * Ax0 + x[1] * Ax1) + x[2] * Ax2) + 2.0 * ((q[6] * x[0] + q[7] * x[1]) + q[8] * x[2])) + q[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.position[p * 3 + k] = a.centre[p * 3 + k] + x[k];
        a.status[p] = (uint8_t)status;
        a.error[p] = e > 0.0 ? e : 0.0;                                   // (NaN fails the comparison)
        a.trace[p] = (q[0] + q[3]) + q[5];
    }
}

__global__ void octree_select_kernel(VdnOctreeSelectArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < (long)a.C; p += stride) {
        const double tr = a.trace[p];
        bool solid = tr > 0.0 && tr < INFINITY && a.error[p] < a.tolerance2 * tr;
        for (int s = 0; s < 8; ++s) {
            const long c = (long)a.children[p * 8 + s];
            if (c >= 0 && c < (long)a.Cc && a.child_solid[c] == 0) solid = false;
        }
        a.solid[p] = solid ? 1 : 0;
    }
}

__global__ void octree_assign_kernel(VdnOctreeAssignArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < (long)a.C0; c += stride) {
        long n = c;
        int level = 0;
        while (level < a.levels) {
            const long up = (long)a.parent[n];
            if (up < 0 || up >= (long)a.N || a.solid[up] == 0) break;
            n = up;
            ++level;
        }
        a.level[c] = (uint8_t)level;
        a.node[c] = n - (long)a.level_start[level];
    }
}

}  // namespace vdn

// 256-thread blocks, grid-stride loops: enough blocks to cover n once, capped at a few waves of the 256 CUs
static inline unsigned grid_of(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

static inline bool index_bytes_ok(int b) { return b == 4 || b == 8; }

static int simplify_check(const VdnSimplifyArgs* a) {
    if (a == nullptr || a->vertices == nullptr || a->V < 1 || a->F < 0) return -1;
    if (a->V > INT_MAX || a->F > INT_MAX) return -10;
    return 0;
}

extern "C" int vdn_simplify_mark(const VdnSimplifyArgs* a, void* stream) {
    const int rc = simplify_check(a);
    if (rc != 0) return rc;
    if (a->triangles == nullptr || a->live == nullptr || a->vertex_used == nullptr || a->error == nullptr || a->F < 1 ||
        !index_bytes_ok(a->index_bytes)) return -1;
    hipLaunchKernelGGL(vdn::simplify_mark_kernel, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_simplify_keys(const VdnSimplifyArgs* a, void* stream) {
    const int rc = simplify_check(a);
    if (rc != 0) return rc;
    if (a->key == nullptr || !(a->h > 0.0) || a->nx < 1 || a->ny < 1 || a->nz < 1) return -1;
    // the key must fit an int64 with room to spare: nx * ny * nz < 2^62
    const double cells = (double)a->nx * (double)a->ny * (double)a->nz;
    if (!(cells < 4611686018427387904.0)) return -1;
    hipLaunchKernelGGL(vdn::simplify_keys_kernel, dim3(grid_of(a->V)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_simplify_records(const VdnSimplifyArgs* a, void* stream) {
    const int rc = simplify_check(a);
    if (rc != 0) return rc;
    if (a->triangles == nullptr || a->live == nullptr || a->vertex_cluster == nullptr || a->corner_cluster == nullptr ||
        a->canonical == nullptr || a->survive == nullptr || a->F < 1 || a->C < 1 || a->C > a->V || !index_bytes_ok(a->index_bytes)) return -1;
    hipLaunchKernelGGL(vdn::simplify_records_kernel, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

// a wave per segment: four segments per 256-thread block
static inline unsigned wave_grid_of(long segments) { return grid_of(segments * 64); }

extern "C" int vdn_segment_mean(const VdnSegmentMeanArgs* a, void* stream) {
    if (a == nullptr || a->rows == nullptr || a->members == nullptr || a->start == nullptr || a->out == nullptr || a->N < 1 ||
        a->M < 0 || a->C < 1 || a->K < 1) return -1;
    if (a->N > INT_MAX || a->M > INT_MAX || a->C > INT_MAX || a->N * (int64_t)a->K > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::segment_mean_kernel, dim3(wave_grid_of(a->C)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

static int quadric_check(const VdnClusterQuadricArgs* a) {
    if (a == nullptr || a->centre == nullptr || a->quadric == nullptr || a->C < 1) return -1;
    if (a->C > INT_MAX || a->V > INT_MAX || a->F > INT_MAX) return -10;
    return 0;
}

extern "C" int vdn_cluster_quadrics(const VdnClusterQuadricArgs* a, void* stream) {
    const int rc = quadric_check(a);
    if (rc != 0) return rc;
    if (a->vertices == nullptr || a->triangles == nullptr || a->members == nullptr || a->start == nullptr || a->V < 1 || a->F < 1 ||
        a->M < 0 || a->M > 3 * a->F || !index_bytes_ok(a->index_bytes)) return -1;
    hipLaunchKernelGGL(vdn::cluster_quadrics_kernel, dim3(wave_grid_of(a->C)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_cluster_place(const VdnClusterQuadricArgs* a, void* stream) {
    const int rc = quadric_check(a);
    if (rc != 0) return rc;
    if (a->mean == nullptr || a->position == nullptr || a->status == nullptr || !(a->h > 0.0) || !(a->eps > 0.0)) return -1;
    hipLaunchKernelGGL(vdn::cluster_place_kernel, dim3(grid_of(a->C)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_octree_merge(const VdnOctreeMergeArgs* a, void* stream) {
    if (a == nullptr || a->centre == nullptr || a->quadric == nullptr || a->mean == nullptr || a->position == nullptr ||
        a->status == nullptr || a->error == nullptr || a->trace == nullptr || a->C < 1 || !(a->h > 0.0) || !(a->eps > 0.0)) return -1;
    if (a->children != nullptr &&
        (a->cell == nullptr || a->child_key == nullptr || a->child_quadric == nullptr || a->child_mean == nullptr ||
         a->child_count == nullptr || a->count == nullptr || a->Cc < 1 || a->nx < 1 || a->ny < 1 || a->nz < 1 ||
         !((double)a->nx * (double)a->ny * (double)a->nz < 4611686018427387904.0))) return -1;
    if (a->C > INT_MAX || a->Cc > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::octree_merge_kernel, dim3(grid_of(a->C)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_octree_select(const VdnOctreeSelectArgs* a, void* stream) {
    if (a == nullptr || a->error == nullptr || a->trace == nullptr || a->children == nullptr || a->child_solid == nullptr ||
        a->solid == nullptr || a->C < 1 || a->Cc < 1 || !(a->tolerance2 >= 0.0)) return -1;
    if (a->C > INT_MAX || a->Cc > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::octree_select_kernel, dim3(grid_of(a->C)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_octree_assign(const VdnOctreeAssignArgs* a, void* stream) {
    if (a == nullptr || a->parent == nullptr || a->solid == nullptr || a->level_start == nullptr || a->level == nullptr ||
        a->node == nullptr || a->C0 < 1 || a->N < a->C0 || a->levels < 1 || a->levels > 8) return -1;
    if (a->N > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::octree_assign_kernel, dim3(grid_of(a->C0)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
