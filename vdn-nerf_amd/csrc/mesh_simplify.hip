// Mesh simplification on the device (include/vdn_render.h: vdn_simplify_*, vdn_segment_mean, vdn_cluster_*): vertex clustering on a
// uniform grid with quadric error placement (vdn_hip/mesh.py: cluster_quadrics, simplify_mesh). A mark pass and a key
// pass per triangle / vertex, the corner records per triangle, then two segmented sums - a wave per cluster, lanes striding the
// cluster's list, a fixed-order tree across the lanes - and one thread per cluster for the 3 x 3 solve. All arithmetic is double on
// the widened fp32 vertices; the file is built with -ffp-contract=off, so every product and sum rounds on its own and a numpy model
// can follow the sums to the bit. No float atomics, no LDS.
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

__global__ void cluster_place_kernel(VdnClusterQuadricArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < (long)a.C; s += stride) {
        const double* q = a.quadric + s * 10;
        const double m[3] = {a.mean[s * 3 + 0], a.mean[s * 3 + 1], a.mean[s * 3 + 2]};
        double x[3] = {m[0], m[1], m[2]};
        int status = 0;
        const double tr = (q[0] + q[3]) + q[5];
        if (!(tr > 0.0 && tr < INFINITY)) {
            status = 1;
        } else {
            const double r = a.eps * tr;
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
            const double half = 0.5 * a.h;
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) ok = ok && fabs(y[k]) <= half;          // (NaN fails the comparison)
            if (ok) { x[0] = y[0]; x[1] = y[1]; x[2] = y[2]; }
            else status = 2;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.position[s * 3 + k] = a.centre[s * 3 + k] + x[k];
        a.status[s] = (uint8_t)status;
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
