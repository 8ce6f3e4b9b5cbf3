// Image evaluation on the device (include/vdn_render.h: vdn_image_stats): the sums behind L1, PSNR and SSIM of a
// rendered image against its ground truth, masked and unmasked, in one pass over the two images. Everything is double on the widened
// fp32 inputs (the file is compiled with -ffp-contract=off): a product of two fp32 values is exact in double, so only the sums round,
// and SSIM's variances - differences of nearly equal numbers on a white background - keep their digits.
//
// One 256-thread workgroup per tile of 16 x 32 valid window centres. It stages the 26 x 42 pixels under the tile's windows (the tile
// and its 5-pixel halo) of both images in LDS, reading each image row as the flat span of 3 * 42 floats it is, then takes the three
// channels in turn: a horizontal 11-tap pass over the five moments x, y, xx, yy, xy of all 26 rows into five double planes, a
// vertical pass over those planes at the tile's centres, S from the ten sums. LDS: 2 * 26 * 126 * 4 (images) + 5 * 26 * 32 * 8 (planes)
// + 26 * 42 (mask bits) + 4 * 9 * 8 (wave sums) = 60 868 bytes: two workgroups share a CU's 160 KiB.
// The pixel sums (|e|, e^2, mask count) are taken over the staged pixels a tile owns: pixel (y, x) belongs to the tile of the
// centre (clamp(y - 5), clamp(x - 5)), so every pixel of the image is counted exactly once.
// Sums: each thread adds its items in a fixed order, the 64 lanes of a wave by a butterfly (every step adds the same two numbers in
// both lanes), the four waves in order; a second launch of one wave adds the tiles lane-strided and then by the same butterfly.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cmath>
#include "vdn_render.h"

namespace vdn {

constexpr int kImgR = 5, kImgTaps = 2 * kImgR + 1;
constexpr int kImgTH = 16, kImgTW = 32;                                   // valid centres per tile
constexpr int kImgIH = kImgTH + 2 * kImgR, kImgIW = kImgTW + 2 * kImgR;  // staged pixels per tile
constexpr int kImgThreads = 256, kImgWaves = kImgThreads / 64;
constexpr int kImgSums = 9;                                               // result[0..8]; result[9] = H W is the finish launch's

struct ImgTaps {
    double w[kImgTaps];
};

// the sum over the 64 lanes of a wave, the same bits in every lane and on every call
__device__ inline double img_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(kImgThreads) void image_stats_kernel(VdnImageStatsArgs a, ImgTaps g) {
    __shared__ float sp[kImgIH][kImgIW * 3], sg[kImgIH][kImgIW * 3];
    __shared__ unsigned char sm[kImgIH][kImgIW];
    __shared__ double pl[5][kImgIH][kImgTW];
    __shared__ double red[kImgWaves][kImgSums];
    const int tid = threadIdx.x;
    const int Hv = a.H - 2 * kImgR, Wv = a.W - 2 * kImgR;
    // the tile's first valid centre, in centre coordinates = its first staged pixel, in image coordinates
    const int y0 = blockIdx.y * kImgTH, x0 = blockIdx.x * kImgTW;
    const int rows = min(kImgIH, a.H - y0), cols = min(kImgIW, a.W - x0);

    for (int i = tid; i < kImgIH * kImgIW * 3; i += kImgThreads) {
        const int ly = i / (kImgIW * 3), j = i - ly * (kImgIW * 3);
        float p = 0.0f, q = 0.0f;                        // (outside the image: read by no valid centre)
        if (ly < rows && j < cols * 3) {
            const size_t src = ((size_t)(y0 + ly) * a.W + x0) * 3 + j;
            p = a.pred[src];
            q = a.gt[src];
        }
        sp[ly][j] = p;
        sg[ly][j] = q;
    }
    __syncthreads();

    double acc[kImgSums];
#pragma unroll
    for (int j = 0; j < kImgSums; ++j) acc[j] = 0.0;

    // the pixel sums of the pixels this tile owns, and the mask bits of all staged pixels
    for (int i = tid; i < kImgIH * kImgIW; i += kImgThreads) {
        const int ly = i / kImgIW, lx = i - ly * kImgIW;
        bool m = false;
        if (ly < rows && lx < cols) {
            const int gy = y0 + ly, gx = x0 + lx;
            m = a.mask == nullptr || (double)a.mask[((size_t)gy * a.W + gx) * a.mask_ch] > 0.1;
            const int cy = min(max(gy - kImgR, 0), Hv - 1), cx = min(max(gx - kImgR, 0), Wv - 1);
            if (cy >= y0 && cy < y0 + kImgTH && cx >= x0 && cx < x0 + kImgTW) {
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double e = (double)sp[ly][lx * 3 + c] - (double)sg[ly][lx * 3 + c];
                    s1 += fabs(e);
                    s2 += e * e;
                }
                acc[3] += s1;
                acc[4] += s2;
                if (m) {
                    acc[0] += 1.0;
                    acc[1] += s1;
                    acc[2] += s2;
                }
            }
        }
        sm[ly][lx] = m ? 1 : 0;
    }

    constexpr int kOut = kImgTH * kImgTW / kImgThreads;          // centres per thread
    double s3[kOut];
#pragma unroll
    for (int t = 0; t < kOut; ++t) s3[t] = 0.0;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < kImgIH * kImgTW; i += kImgThreads) {
            const int ly = i / kImgTW, lx = i - ly * kImgTW;
            double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
            for (int k = 0; k < kImgTaps; ++k) {
                const double x = (double)sp[ly][(lx + k) * 3 + c], y = (double)sg[ly][(lx + k) * 3 + c], w = g.w[k];
                mx += w * x;
                my += w * y;
                xx += w * (x * x);
                yy += w * (y * y);
                xy += w * (x * y);
            }
            pl[0][ly][lx] = mx;
            pl[1][ly][lx] = my;
            pl[2][ly][lx] = xx;
            pl[3][ly][lx] = yy;
            pl[4][ly][lx] = xy;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kOut; ++t) {
            const int i = tid + t * kImgThreads;
            const int oy = i / kImgTW, ox = i - oy * kImgTW;
            if (y0 + oy < Hv && x0 + ox < Wv) {
                double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
                for (int k = 0; k < kImgTaps; ++k) {
                    const double w = g.w[k];
                    mx += w * pl[0][oy + k][ox];
                    my += w * pl[1][oy + k][ox];
                    xx += w * pl[2][oy + k][ox];
                    yy += w * pl[3][oy + k][ox];
                    xy += w * pl[4][oy + k][ox];
                }
                // x == y makes mx == my and xx == yy == xy bit for bit, and then the two products below: S == 1
                const double mxx = mx * mx, myy = my * my, mxy = mx * my;
                const double vx = xx - mxx, vy = yy - myy, vxy = xy - mxy;
                const double num = (2.0 * mxy + C1) * (2.0 * vxy + C2);
                const double den = ((mxx + myy) + C1) * ((vx + vy) + C2);
                s3[t] += num / den;
            }
        }
        __syncthreads();                                         // the planes are rewritten by the next channel
    }

#pragma unroll
    for (int t = 0; t < kOut; ++t) {
        const int i = tid + t * kImgThreads;
        const int oy = i / kImgTW, ox = i - oy * kImgTW;
        if (y0 + oy < Hv && x0 + ox < Wv) {
            if (a.ssim_map != nullptr) a.ssim_map[(size_t)(y0 + oy) * Wv + (x0 + ox)] = (float)(s3[t] / 3.0);
            acc[5] += s3[t];
            acc[6] += 1.0;
            if (sm[oy + kImgR][ox + kImgR]) {
                acc[7] += s3[t];
                acc[8] += 1.0;
            }
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < kImgSums; ++j) {
        const double v = img_wave_sum(acc[j]);
        if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
    if (tid < kImgSums) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < kImgWaves; ++w) v += red[w][tid];
        a.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kImgSums + tid] = v;
    }
}

// one wave: lane l adds tiles l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void image_stats_finish_kernel(const double* partials, int n_tiles, double n_pixels, double* result) {
    const int lane = threadIdx.x;
    double acc[kImgSums];
#pragma unroll
    for (int j = 0; j < kImgSums; ++j) acc[j] = 0.0;
    for (int t = lane; t < n_tiles; t += 64) {
#pragma unroll
        for (int j = 0; j < kImgSums; ++j) acc[j] += partials[(size_t)t * kImgSums + j];
    }
#pragma unroll
    for (int j = 0; j < kImgSums; ++j) {
        const double v = img_wave_sum(acc[j]);
        if (lane == 0) result[j] = v;
    }
    if (lane == 0) result[kImgSums] = n_pixels;
}

}  // namespace vdn

static inline int img_tiles_1d(int n_valid, int tile) { return (n_valid + tile - 1) / tile; }

extern "C" int vdn_image_stats_tiles(int32_t H, int32_t W) {
    if (H < vdn::kImgTaps || W < vdn::kImgTaps || (int64_t)H * W > INT_MAX) return 0;
    return img_tiles_1d(H - 2 * vdn::kImgR, vdn::kImgTH) * img_tiles_1d(W - 2 * vdn::kImgR, vdn::kImgTW);
}

extern "C" int vdn_image_stats(const VdnImageStatsArgs* a, void* stream) {
    if (a == nullptr || a->pred == nullptr || a->gt == nullptr || a->result == nullptr || a->partials == nullptr ||
        a->H < vdn::kImgTaps || a->W < vdn::kImgTaps) return -1;
    if (a->mask != nullptr && a->mask_ch != 1 && a->mask_ch != 3) return -1;
    if ((int64_t)a->H * a->W > INT_MAX) return -10;
    const int ty = img_tiles_1d(a->H - 2 * vdn::kImgR, vdn::kImgTH), tx = img_tiles_1d(a->W - 2 * vdn::kImgR, vdn::kImgTW);
    if (ty > 65535 || (int64_t)ty * tx > INT_MAX) return -10;
    if (a->partials_rows < (int64_t)ty * tx) return -1;
    vdn::ImgTaps g;
    double sum = 0.0;
    for (int k = 0; k < vdn::kImgTaps; ++k) {
        const double d = (double)(k - vdn::kImgR);
        g.w[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g.w[k];
    }
    for (int k = 0; k < vdn::kImgTaps; ++k) g.w[k] /= sum;
    hipLaunchKernelGGL(vdn::image_stats_kernel, dim3(tx, ty), dim3(vdn::kImgThreads), 0, (hipStream_t)stream, *a, g);
    hipLaunchKernelGGL(vdn::image_stats_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)a->partials, ty * tx,
                       (double)a->H * (double)a->W, a->result);
    return (int)hipGetLastError();
}
