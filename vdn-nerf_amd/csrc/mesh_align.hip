// Mesh alignment on the device (include/vdn_render.h: vdn_icp_round): one round of ICP from surface samples to a
// scanned cloud in one pass - transform a sample, find its nearest scan point on the scan's uniform grid (k_nn.h: vdn_nn_query's own
// search), and reduce the matched pairs to the 19 moments a closed-form similarity solve needs. Gather-bound scalar work like
// mesh_eval.hip: one lane per sample, no LDS but the 4 x 19 doubles of the workgroup's sums.
// The double arithmetic is compiled with -ffp-contract=off (vdn_hip/build.py): a product of two widened fp32 values is exact, so
// only the documented sums round and a numpy model reproduces y and every term bit for bit; the fp32 search keeps vdn_nn_query's
// contraction (k_nn.h).
// Sums: a lane has one pair's terms (zeros without a pair), the 64 lanes of a wave add by a butterfly (every step adds the same two
// numbers in both lanes), the four waves in order; a second launch of one workgroup adds the blocks, thread-strided, then the same
// way. No atomics, no early return before the reduction: every lane of every wave takes part in every shuffle.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cmath>
#include "vdn_render.h"
#include "k_nn.h"

namespace vdn {

constexpr int kIcpThreads = 256, kIcpWaves = kIcpThreads / 64;
constexpr int kIcpSums = VDN_ICP_SUMS;

// the sum over the 64 lanes of a wave, the same bits in every lane and on every call
__device__ inline double icp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// acc[19] of every thread of the workgroup -> out[19]: the lanes of a wave by the butterfly, the waves in wave order
__device__ inline void icp_block_sum(const double* acc, double (*red)[kIcpSums], double* out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < kIcpSums; ++j) {
        const double v = icp_wave_sum(acc[j]);
        if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
    if (tid < kIcpSums) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < kIcpWaves; ++w) v += red[w][tid];
        out[tid] = v;
    }
}

__global__ __launch_bounds__(kIcpThreads) void icp_round_kernel(VdnIcpArgs a) {
    __shared__ double red[kIcpWaves][kIcpSums];
    const long t = (long)blockIdx.x * kIcpThreads + threadIdx.x;
    double acc[kIcpSums];
#pragma unroll
    for (int j = 0; j < kIcpSums; ++j) acc[j] = 0.0;
    long i = -1;
    if (t < (long)a.N) {
        i = a.order != nullptr ? (long)a.order[t] : t;
        if (i < 0 || i >= (long)a.N) i = -1;               // (an index outside the cloud reads and writes nothing)
    }
    if (i >= 0) {
        const float pxf = a.src[i * 3 + 0], pyf = a.src[i * 3 + 1], pzf = a.src[i * 3 + 2];
        const double px = (double)pxf, py = (double)pyf, pz = (double)pzf;
        const float yx = (float)(((a.m00 * px + a.m01 * py) + a.m02 * pz) + a.m03);
        const float yy = (float)(((a.m10 * px + a.m11 * py) + a.m12 * pz) + a.m13);
        const float yz = (float)(((a.m20 * px + a.m21 * py) + a.m22 * pz) + a.m23);
        NnBest b;
        nn_search(a, yx, yy, yz, b);
        float d;
        const bool hit = nn_hit(b, a.max_dist, &d);
        if (a.dist != nullptr) a.dist[i] = hit ? d : INFINITY;
        if (a.idx != nullptr) a.idx[i] = hit ? (int64_t)b.idx : (int64_t)-1;
        if (hit) {
            // the matched record's own coordinates, by the sorted position the search kept
            const float4 r = ((const float4*)a.ref)[b.at];
            const double qx = (double)r.x, qy = (double)r.y, qz = (double)r.z;
            const double ex = (double)yx - qx, ey = (double)yy - qy, ez = (double)yz - qz;
            acc[VDN_ICP_N] = 1.0;
            acc[VDN_ICP_P + 0] = px;
            acc[VDN_ICP_P + 1] = py;
            acc[VDN_ICP_P + 2] = pz;
            acc[VDN_ICP_Q + 0] = qx;
            acc[VDN_ICP_Q + 1] = qy;
            acc[VDN_ICP_Q + 2] = qz;
            acc[VDN_ICP_PP] = (px * px + py * py) + pz * pz;
            acc[VDN_ICP_QQ] = (qx * qx + qy * qy) + qz * qz;
            acc[VDN_ICP_QP + 0] = qx * px;
            acc[VDN_ICP_QP + 1] = qx * py;
            acc[VDN_ICP_QP + 2] = qx * pz;
            acc[VDN_ICP_QP + 3] = qy * px;
            acc[VDN_ICP_QP + 4] = qy * py;
            acc[VDN_ICP_QP + 5] = qy * pz;
            acc[VDN_ICP_QP + 6] = qz * px;
            acc[VDN_ICP_QP + 7] = qz * py;
            acc[VDN_ICP_QP + 8] = qz * pz;
            acc[VDN_ICP_RES] = (ex * ex + ey * ey) + ez * ez;
        }
    }
    // every lane of the workgroup is here (no return above)
    icp_block_sum(acc, red, a.partials + (size_t)blockIdx.x * kIcpSums);
}

// one workgroup: thread j adds blocks j, j + 256, .. in order, then the workgroup's sum as above
__global__ __launch_bounds__(kIcpThreads) void icp_finish_kernel(const double* partials, int n_blocks, double* result) {
    __shared__ double red[kIcpWaves][kIcpSums];
    double acc[kIcpSums];
#pragma unroll
    for (int j = 0; j < kIcpSums; ++j) acc[j] = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += kIcpThreads) {
#pragma unroll
        for (int j = 0; j < kIcpSums; ++j) acc[j] += partials[(size_t)b * kIcpSums + j];
    }
    icp_block_sum(acc, red, result);
}

}  // namespace vdn

extern "C" int vdn_icp_round_blocks(int64_t N) {
    if (N < 1 || N > INT_MAX) return 0;
    return (int)((N + vdn::kIcpThreads - 1) / vdn::kIcpThreads);
}

extern "C" int vdn_icp_round(const VdnIcpArgs* a, void* stream) {
    if (a == nullptr || a->src == nullptr || a->ref == nullptr || a->cell_start == nullptr || a->partials == nullptr ||
        a->result == nullptr || a->N < 1 || a->R < 1 || a->nx < 1 || a->ny < 1 || a->nz < 1 || !(a->h > 0.0f) || !(a->h < INFINITY) ||
        !(a->margin >= 0.0f) || !(a->max_dist >= 0.0f)) return -1;
    const double m[12] = {a->m00, a->m01, a->m02, a->m03, a->m10, a->m11, a->m12, a->m13, a->m20, a->m21, a->m22, a->m23};
    for (int j = 0; j < 12; ++j)
        if (!std::isfinite(m[j])) return -1;
    if (a->N > INT_MAX || a->R > INT_MAX || (int64_t)a->nx * a->ny * a->nz >= (int64_t)INT_MAX) return -10;
    const int blocks = vdn_icp_round_blocks(a->N);
    if (a->partials_rows < (int64_t)blocks) return -1;
    hipLaunchKernelGGL(vdn::icp_round_kernel, dim3(blocks), dim3(vdn::kIcpThreads), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(vdn::icp_finish_kernel, dim3(1), dim3(vdn::kIcpThreads), 0, (hipStream_t)stream, (const double*)a->partials, blocks,
                       a->result);
    return (int)hipGetLastError();
}
