// The exact nearest-neighbour search on the uniform grid, shared by vdn_nn_query and vdn_thin_round (mesh_eval.hip) and by
// vdn_icp_round (mesh_align.hip): the cell coordinate of a point, the scan of one x-row's records and the Chebyshev shell loop with
// its stop rule. `A` is an argument block with the grid's fields under vdn_nn_query's names (ref, cell_start, R, lo_*, h, margin,
// max_dist, nx, ny, nz: VdnNnArgs, VdnIcpArgs).
//
// The fp32 expressions here are compiled under `fp contract(fast)` whatever the including file's -ffp-contract says: it is
// hipcc's default, what vdn_nn_query has always been built with, and a file that turns contraction off for its own double
// arithmetic (mesh_align.hip) still gets the same squared distances, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>

namespace vdn {

// cell coordinate along one axis: floor((p - lo) / h) in fp32, clamped into the grid (a point outside, or NaN, lands in a border cell)
__device__ inline int nn_axis(float p, float lo, float h, int n) {
#pragma clang fp contract(fast)
    const float t = (p - lo) / h;
    return (int)fminf(fmaxf(floorf(t), 0.0f), (float)(n - 1));
}

struct NnBest {
    float d2;
    int idx;                       // the record's original index
    int at;                        // its position in the sorted reference
};

// the records of cells [c0, c1] of one x-row (contiguous in the sorted reference), against the query
template <class A>
__device__ inline void nn_scan(const A& a, int c0, int c1, float qx, float qy, float qz, NnBest& b) {
#pragma clang fp contract(fast)
    const int begin = max(a.cell_start[c0], 0), end = min(a.cell_start[c1 + 1], (int)a.R);
    const float4* rec = (const float4*)a.ref;
    for (int r = begin; r < end; ++r) {
        const float4 p = rec[r];                       // one 16-byte load: x, y, z, original index
        const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const int id = __float_as_int(p.w);
        // ties go to the lower original index, so the answer does not depend on the order cells are visited in
        if (d2 < b.d2 || (d2 == b.d2 && id < b.idx)) { b.d2 = d2; b.idx = id; b.at = r; }
    }
}

// the nearest record of the query (qx, qy, qz) into `b` (idx INT_MAX: the grid is empty) -> the last shell visited
template <class A>
__device__ inline int nn_search(const A& a, float qx, float qy, float qz, NnBest& b) {
#pragma clang fp contract(fast)
    const int cx = nn_axis(qx, a.lo_x, a.h, a.nx), cy = nn_axis(qy, a.lo_y, a.h, a.ny), cz = nn_axis(qz, a.lo_z, a.h, a.nz);
    // the last shell that still touches the grid
    const int k_last = max(max(max(cx, a.nx - 1 - cx), max(cy, a.ny - 1 - cy)), max(cz, a.nz - 1 - cz));
    b = {INFINITY, INT_MAX, 0};
    int k = 0;
    for (;; ++k) {
        // Chebyshev shell k: rows (y, z) on the shell's y / z faces take the whole x-range, the others its two end cells
        const int x0 = max(cx - k, 0), x1 = min(cx + k, a.nx - 1);
        for (int z = max(cz - k, 0); z <= min(cz + k, a.nz - 1); ++z) {
            for (int y = max(cy - k, 0); y <= min(cy + k, a.ny - 1); ++y) {
                const int row = (z * a.ny + y) * a.nx;
                if (abs(z - cz) == k || abs(y - cy) == k) {
                    nn_scan(a, row + x0, row + x1, qx, qy, qz, b);
                } else {
                    if (cx - k >= 0) nn_scan(a, row + cx - k, row + cx - k, qx, qy, qz, b);
                    if (cx + k < a.nx) nn_scan(a, row + cx + k, row + cx + k, qx, qy, qz, b);
                }
            }
        }
        if (k >= k_last) break;
        // every point in a cell at index distance >= k + 1 is at least k h away, less the fp32 rounding of the binning: `margin`
        const float r = (float)k * a.h - a.margin;
        if (r > 0.0f && (b.d2 <= r * r || r >= a.max_dist)) break;
    }
    return k;
}

// the search's answer in vdn_nn_query's format: d = sqrtf(d2), a hit when a record was seen and d <= max_dist (inclusive)
__device__ inline bool nn_hit(const NnBest& b, float max_dist, float* d) {
    *d = sqrtf(b.d2);
    return b.idx != INT_MAX && *d <= max_dist;
}

}  // namespace vdn
