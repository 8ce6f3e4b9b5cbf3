// Mesh cleaning on the device (include/vdn_render.h: vdn_cc_*, vdn_tri_area, vdn_mask_*, vdn_mesh_filter_*): connected components
// of a triangle mesh by a lock-free union-find over its index buffer, per-face areas, mask dilation and per-vertex mask votes, and
// the two passes of face / vertex compaction (vdn_hip/mesh.py, vdn_train/mesh_clean.py). Gather-bound integer work, no LDS: one
// thread per triangle, vertex or pixel. The prefix sums between the compaction passes are the caller's torch ops.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include "vdn_render.h"
#include "k_tri.h"
#include "k_project.h"

namespace vdn {

// ---- connected components ---------------------------------------------------------------------------------------------------------
// parent[x] <= x at all times and a slot changes only (a) by the hook - a compare-and-swap on a ROOT's own slot, parent[r] == r, to a
// smaller root - or (b) by path halving - an atomic minimum with an ancestor on a slot that is no root any more. Both lower the
// value, so every value read is an ancestor of its slot (possibly an old one), every chain ends at a root, and the root of a tree is
// its smallest vertex.
__device__ inline int cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; chains longer than one step are halved on the way (the only stores of the find loop: none once the paths are short)
__device__ inline int cc_find(int32_t* parent, int x) {
    int p = cc_load(parent + x);
    while (p != x) {
        const int g = cc_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// a failed compare-and-swap returns the slot's new value, a smaller ancestor: the retry starts there, never waits, and every
// round lowers b's root candidate or ends
__device__ inline void cc_join(int32_t* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int seen = atomicCAS(parent + b, b, a);          // the larger root under the smaller, on the root's own slot
        if (seen == b) return;
        b = seen;
    }
}

__global__ void cc_union_kernel(VdnCcArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < (long)a.F; f += stride) {
        long i[3];
        if (!tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i)) {
            *a.error = 1;              // (every writer stores the same word); the triangle joins nothing
            continue;
        }
        if (i[0] != i[1]) cc_join(a.parent, (int)i[0], (int)i[1]);
        if (i[1] != i[2]) cc_join(a.parent, (int)i[1], (int)i[2]);
    }
}

__global__ void cc_flatten_kernel(VdnCcArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < (long)a.V; v += stride) {
        int x = (int)v, p = a.parent[x];
        while (p != x) { x = p; p = a.parent[x]; }            // (the union launch has ended: plain loads, nothing is written to parent)
        a.label[v] = x;
    }
}

// ---- per-face area ----------------------------------------------------------------------------------------------------------------
__global__ void tri_area_kernel(VdnTriAreaArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < (long)a.F; f += stride) {
        long i[3];
        double area = 0.0;
        if (!tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i)) *a.error = 1;
        else area = tri_area(a.vertices, i);
        a.area[f] = area < INFINITY ? area : 0.0;             // (NaN fails the comparison)
    }
}

// ---- mask dilation: window maximum along one axis ------------------------------------------------------------------------------------
template <bool ROWS>
__global__ void mask_dilate_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long n_pixels, int H, int W, int r) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pixels; i += stride) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        int m = 0;
        if (ROWS) {
            const uint8_t* row = src + (i - x);
            for (int k = max(x - r, 0); k <= min(x + r, W - 1); ++k) m = max(m, (int)row[k]);
        } else {
            const uint8_t* col = src + (i - (long)y * W);
            for (int k = max(y - r, 0); k <= min(y + r, H - 1); ++k) m = max(m, (int)col[(long)k * W]);
        }
        dst[i] = (uint8_t)m;
    }
}

// ---- mask votes -------------------------------------------------------------------------------------------------------------------
__global__ void mask_votes_kernel(VdnMaskVotesArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < (long)a.V; v += stride) {
        const double x = (double)a.vertices[v * 3 + 0], y = (double)a.vertices[v * 3 + 1], z = (double)a.vertices[v * 3 + 2];
        int n_img = 0, n_msk = 0;
        for (long n = 0; n < (long)a.N; ++n) {
            long px, py;                                     // (P is uniform over the wave: scalar loads)
            if (!project_in_image(a.P + n * 12, x, y, z, a.H, a.W, &px, &py)) continue;
            ++n_img;
            n_msk += a.masks[(n * a.H + py) * a.W + px] != 0 ? 1 : 0;
        }
        a.n_in_image[v] = n_img;
        a.n_in_mask[v] = n_msk;
    }
}

// ---- compaction -------------------------------------------------------------------------------------------------------------------
__global__ void mesh_filter_mark_kernel(VdnMeshFilterArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < (long)a.F; f += stride) {
        long i[3];
        bool alive = a.keep_face == nullptr || a.keep_face[f] != 0;
        if (!tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i)) {
            *a.error = 1;
            alive = false;
        } else if (alive && a.keep_vertex != nullptr) {
            alive = a.keep_vertex[i[0]] != 0 && a.keep_vertex[i[1]] != 0 && a.keep_vertex[i[2]] != 0;
        }
        a.face_alive[f] = alive ? 1 : 0;
        if (alive) a.vertex_used[i[0]] = a.vertex_used[i[1]] = a.vertex_used[i[2]] = 1;      // (plain stores of one value: order-free)
    }
}

__global__ void mesh_filter_remap_kernel(VdnMeshFilterArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < (long)a.F; f += stride) {
        if (a.face_alive[f] == 0) continue;
        long i[3];
        if (!tri_corners(a.triangles, a.index_bytes, (long)a.V, f, i)) continue;     // (never alive: the mark pass cleared it)
        const long o = (long)a.face_offsets[f];
        if (o < 0 || o >= (long)a.F_out) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t n = a.vertex_new[i[c]];
            if (a.index_bytes == 8) ((int64_t*)a.out_triangles)[o * 3 + c] = n;
            else ((int32_t*)a.out_triangles)[o * 3 + c] = (int32_t)n;
        }
    }
}

}  // namespace vdn

// 256-thread blocks, grid-stride loops: enough blocks to cover n once, capped at a few waves of the 256 CUs
static inline unsigned grid_of(long n) {
    const long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

static inline bool index_bytes_ok(int b) { return b == 4 || b == 8; }

static int cc_check(const VdnCcArgs* a) {
    if (a == nullptr || a->parent == nullptr || a->V < 1 || a->F < 0) return -1;
    if (a->V > INT_MAX || a->F > INT_MAX) return -10;
    return 0;
}

extern "C" int vdn_cc_union(const VdnCcArgs* a, void* stream) {
    const int rc = cc_check(a);
    if (rc != 0) return rc;
    if (a->triangles == nullptr || a->error == nullptr || a->F < 1 || !index_bytes_ok(a->index_bytes)) return -1;
    hipLaunchKernelGGL(vdn::cc_union_kernel, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_cc_flatten(const VdnCcArgs* a, void* stream) {
    const int rc = cc_check(a);
    if (rc != 0) return rc;
    if (a->label == nullptr) return -1;
    hipLaunchKernelGGL(vdn::cc_flatten_kernel, dim3(grid_of(a->V)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_tri_area(const VdnTriAreaArgs* a, void* stream) {
    if (a == nullptr || a->vertices == nullptr || a->triangles == nullptr || a->area == nullptr || a->error == nullptr || a->F < 1 ||
        a->V < 1 || !index_bytes_ok(a->index_bytes)) return -1;
    if (a->V > INT_MAX || a->F > INT_MAX) return -10;
    hipLaunchKernelGGL(vdn::tri_area_kernel, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

// N * H * W as a 32-bit count, or -1
static long pixel_count(int64_t N, int32_t H, int32_t W) {
    if (N > INT_MAX) return -1;
    const int64_t hw = (int64_t)H * W;
    if (hw > INT_MAX || N * hw > INT_MAX) return -1;
    return (long)(N * hw);
}

extern "C" int vdn_mask_dilate(const VdnMaskDilateArgs* a, void* stream) {
    if (a == nullptr || a->src == nullptr || a->scratch == nullptr || a->dst == nullptr || a->N < 1 || a->H < 1 || a->W < 1 ||
        a->radius < 0 || a->scratch == a->src || a->scratch == a->dst) return -1;
    const long n = pixel_count(a->N, a->H, a->W);
    if (n < 0) return -10;
    hipLaunchKernelGGL(vdn::mask_dilate_kernel<true>, dim3(grid_of(n)), dim3(256), 0, (hipStream_t)stream, a->src, a->scratch, n, a->H, a->W, a->radius);
    hipLaunchKernelGGL(vdn::mask_dilate_kernel<false>, dim3(grid_of(n)), dim3(256), 0, (hipStream_t)stream, a->scratch, a->dst, n, a->H, a->W, a->radius);
    return (int)hipGetLastError();
}

extern "C" int vdn_mask_votes(const VdnMaskVotesArgs* a, void* stream) {
    if (a == nullptr || a->vertices == nullptr || a->P == nullptr || a->masks == nullptr || a->n_in_image == nullptr ||
        a->n_in_mask == nullptr || a->V < 1 || a->N < 1 || a->H < 1 || a->W < 1) return -1;
    if (a->V > INT_MAX || pixel_count(a->N, a->H, a->W) < 0) return -10;
    hipLaunchKernelGGL(vdn::mask_votes_kernel, dim3(grid_of(a->V)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

static int filter_check(const VdnMeshFilterArgs* a) {
    if (a == nullptr || a->triangles == nullptr || a->face_alive == nullptr || a->F < 1 || a->V < 1 || !index_bytes_ok(a->index_bytes)) return -1;
    if (a->V > INT_MAX || a->F > INT_MAX) return -10;
    return 0;
}

extern "C" int vdn_mesh_filter_mark(const VdnMeshFilterArgs* a, void* stream) {
    const int rc = filter_check(a);
    if (rc != 0) return rc;
    if (a->vertex_used == nullptr || a->error == nullptr) return -1;
    hipLaunchKernelGGL(vdn::mesh_filter_mark_kernel, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_mesh_filter_remap(const VdnMeshFilterArgs* a, void* stream) {
    const int rc = filter_check(a);
    if (rc != 0) return rc;
    if (a->face_offsets == nullptr || a->vertex_new == nullptr || a->out_triangles == nullptr || a->F_out < 1 || a->F_out > a->F) return -1;
    hipLaunchKernelGGL(vdn::mesh_filter_remap_kernel, dim3(grid_of(a->F)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
