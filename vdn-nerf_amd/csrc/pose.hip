// Learnable camera poses in the training step (reference dpt_models/poses.py:16-47, 168-212; lie_group_helper.py Exp;
// dataset.py:111-118; renderer.py:335-359 through NeuSRenderer._attach_rays): rays from a camera's (r, t) and the adjoint
// from the ray adjoints back to (r, t). Built with -ffp-contract=off like rays.hip: the fp32 pose and ray expressions round
// like the reference's separate aten ops.
#include "vdn_common.h"
#include "vdn_kernels.h"
#include "k_pixel_gather.h"
#include "k_ray_rows.h"

namespace vdn {

// c2w[:3,:4] = (make_c2w(r, t) @ init_c2w)[:3] in fp32, the reference's expression: K = [r]x, n = |r| + 1e-15,
// R = (I + sin(n)/n K) + (1 - cos n)/n^2 (K @ K)   (no series: at |r| <~ 3e-4 the fp32 cancellation is the reference's own)
VDN_DEV void pose_c2w(const float* rp, const float* tp, const float* init, float c2w[12]) {
    const float r0 = rp[0], r1 = rp[1], r2 = rp[2];
    const float K[9] = {0.0f, -r2, r1, r2, 0.0f, -r0, -r1, r0, 0.0f};
    const float n = sqrtf(r0 * r0 + r1 * r1 + r2 * r2) + 1e-15f;
    const float a = sinf(n) / n;
    const float b = (1.0f - cosf(n)) / (n * n);
    float R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float kk = K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j] + K[i * 3 + 2] * K[2 * 3 + j];
            R[i * 3 + j] = ((i == j ? 1.0f : 0.0f) + a * K[i * 3 + j]) + b * kk;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (init == nullptr) {
#pragma unroll
            for (int j = 0; j < 3; ++j) c2w[i * 4 + j] = R[i * 3 + j];
            c2w[i * 4 + 3] = tp[i];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                c2w[i * 4 + j] = R[i * 3 + 0] * init[0 * 4 + j] + R[i * 3 + 1] * init[1 * 4 + j] + R[i * 3 + 2] * init[2 * 4 + j] +
                                 tp[i] * init[3 * 4 + j];
        }
    }
}

// rays_d = c2w[:3,:3] normalize(K^-1 [x, y, 1]) (poses.py:198-208), v = the camera-frame unit direction
VDN_DEV void pose_ray(const float* Ki, const float* c2w, float x, float y, float v[3], float d[3], float org[3]) {
    float p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = Ki[r * 3 + 0] * x + Ki[r * 3 + 1] * y + Ki[r * 3 + 2];
    const float nrm = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] = p[r] / nrm;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        d[r] = c2w[r * 4 + 0] * v[0] + c2w[r * 4 + 1] * v[1] + c2w[r * 4 + 2] * v[2];
        org[r] = c2w[r * 4 + 3];
    }
}

__global__ __launch_bounds__(256) void gen_rays_pose_kernel(VdnGenRaysPoseArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.B) return;
    float c2w[12];
    pose_c2w(a.r, a.t, a.init_c2w, c2w);
    const float x = a.pixels_x[i], y = a.pixels_y[i];
    float v[3], d[3], org[3];
    pose_ray(a.intrinsic_inv, c2w, x, y, v, d, org);
    float* o = a.out + (long)i * a.out_ld;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[r] = org[r];
        o[3 + r] = d[r];
    }
    gather_pixel_row(a, x, y, o);
    if (a.near != nullptr && a.far != nullptr) {
        const float mid = sphere_mid(org, d);
        a.near[i] = mid - 1.0f;
        a.far[i] = mid + 1.0f;
    }
}

constexpr int kPoseThreads = 256;

// Pass 1, one wave per ray (lanes over the ray's depths: coalesced row reads, spread over the chip): the ray's contribution
// to d c2w[:3,:4] - G_d v^T (9) and G_o (3) - in fp64, written to scratch[b][12].
__global__ __launch_bounds__(kPoseThreads) void pose_ray_terms_kernel(VdnPoseAdjointArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (kPoseThreads / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    float c2w[12];
    pose_c2w(a.r, a.t, a.init_c2w, c2w);
    float v[3], d[3], org[3];
    pose_ray(a.intrinsic_inv, c2w, a.pixels_x[b], a.pixels_y[b], v, d, org);
    const float aa = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float mid = sphere_mid(org, d);
    const float far = mid + 1.0f;
    const float inv_s = 1.0f / (float)a.n_samples;
    // d loss / d near, d far (renderer.py:335-336, 359 as NeuSRenderer._attach_rays attaches them)
    double g_near = 0.0, g_far = 0.0;
    if (a.d_z_out != nullptr) {
        for (int k = lane; k < a.O; k += 64) {
            const long q = (long)b * a.O + k;
            const float c = far != 0.0f ? (a.z_out[q] - inv_s) / far : 0.0f;
            g_far += (double)a.d_z_out[q] * (double)c;
        }
    }
    if (a.n_importance == 0 && a.d_z != nullptr) {
        for (int k = lane; k < a.N; k += 64) {
            const double dz = (double)a.d_z[(long)b * a.N + k], l = (double)a.lin_samples[k];
            g_near += dz * (1.0 - l);
            g_far += dz * l;
        }
    }
    // (a fixed butterfly: the same sums in the same order on every run)
    const double g_mid = wave_sum(g_near) + wave_sum(g_far);
    if (lane != 0) return;
    // near / far -> rays: mid = -(o.d) / (d.d); d mid / d o = -d / aa, d mid / d d = (-o - 2 mid d) / aa
    double* out = a.scratch + (long)b * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double go = (double)a.d_rays_o[b * 3 + r] - g_mid * (double)d[r] / (double)aa;
        const double gd = (double)a.d_rays_d[b * 3 + r] + g_mid * (-(double)org[r] - 2.0 * (double)mid * (double)d[r]) / (double)aa;
#pragma unroll
        for (int j = 0; j < 3; ++j) out[r * 3 + j] = gd * (double)v[j];
        out[9 + r] = go;
    }
}

// Pass 2, one workgroup: the sum over the rays (threads stride the rows in order, then a fixed-order tree in LDS; no atomics:
// bit-reproducible) and the adjoint of the pose itself.
__global__ __launch_bounds__(kPoseThreads) void pose_adjoint_kernel(VdnPoseAdjointArgs a) {
    __shared__ double sh[12][kPoseThreads];
    const int tid = threadIdx.x;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (int b = tid; b < a.B; b += kPoseThreads) {
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[k] += a.scratch[(long)b * 12 + k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) sh[k][tid] = acc[k];
    __syncthreads();
    for (int s = kPoseThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 12; ++k) sh[k][tid] += sh[k][tid + s];
        }
        __syncthreads();
    }
    // dense outputs: zeros outside row `cam` (torch's .grad of LearnPose.r / .t after loss.backward())
    for (int e = tid; e < a.n_cams * 3; e += kPoseThreads) {
        if (e / 3 != a.cam) {
            a.grad_r[e] = 0.0f;
            a.grad_t[e] = 0.0f;
        }
    }
    if (tid != 0) return;
    // d c2w[:3,:4] -> d R, d t through c2w = [R t] @ init_c2w: dR = G init[:3,:]^T, dt = G init[3,:]^T
    double G[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) G[i * 4 + j] = sh[i * 3 + j][0];
        G[i * 4 + 3] = sh[9 + i][0];
    }
    double dR[9], dt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (a.init_c2w == nullptr) {
#pragma unroll
            for (int j = 0; j < 3; ++j) dR[i * 3 + j] = G[i * 4 + j];
            dt[i] = G[i * 4 + 3];
        } else {
            const float* M = a.init_c2w;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += G[i * 4 + k] * (double)M[j * 4 + k];
                dR[i * 3 + j] = s;
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += G[i * 4 + k] * (double)M[3 * 4 + k];
            dt[i] = s;
        }
    }
    // adjoint of Exp: R = I + A(n) K + B(n) K^2, n = |r| + 1e-15.
    // gK = A dR + B (dR K^T + K^T dR); d r = vee(gK) + (ga A'(n) + gb B'(n)) r / |r| (the norm's own path: zero at r = 0, where
    // torch's autograd of the same formula gives dR/dr_k = [e_k]x, as here with A(1e-15) = 1)
    const double r0 = a.r[0], r1 = a.r[1], r2 = a.r[2];
    const double K[9] = {0.0, -r2, r1, r2, 0.0, -r0, -r1, r0, 0.0};
    const double nr = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    const double n = nr + 1e-15;
    const double sn = sin(n), cn = cos(n);
    const double A = sn / n, Bc = (1.0 - cn) / (n * n);
    double gK[9], ga = 0.0, gb = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0, kk = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s += dR[i * 3 + k] * K[j * 3 + k] + K[k * 3 + i] * dR[k * 3 + j];     // (dR K^T + K^T dR)[i][j]
                kk += K[i * 3 + k] * K[k * 3 + j];
            }
            gK[i * 3 + j] = A * dR[i * 3 + j] + Bc * s;
            ga += dR[i * 3 + j] * K[i * 3 + j];
            gb += dR[i * 3 + j] * kk;
        }
    double gr[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
    if (nr > 0.0) {
        const double dA = (n * cn - sn) / (n * n);
        const double dB = (n * sn - 2.0 * (1.0 - cn)) / (n * n * n);
        const double gn = (ga * dA + gb * dB) / nr;
        gr[0] += gn * r0;
        gr[1] += gn * r1;
        gr[2] += gn * r2;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.grad_r[a.cam * 3 + k] = (float)gr[k];
        a.grad_t[a.cam * 3 + k] = (float)dt[k];
    }
}

}  // namespace vdn

using namespace vdn;

extern "C" int vdn_gen_rays_pose(const VdnGenRaysPoseArgs* a, void* stream) {
    if (!a || a->B <= 0 || !a->pixels_x || !a->pixels_y || !a->intrinsic_inv || !a->r || !a->t || !a->out) return -1;
    if (a->out_ld < 6 || a->H <= 0 || a->W <= 0) return -2;
    if (a->feats && (a->C <= 0 || a->out_ld < 10 + a->C)) return -3;
    if (a->mask && a->mask_ch <= 0) return -4;
    hipLaunchKernelGGL(gen_rays_pose_kernel, dim3((a->B + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_pose_adjoint(const VdnPoseAdjointArgs* a, void* stream) {
    if (!a || a->B <= 0 || !a->pixels_x || !a->pixels_y || !a->intrinsic_inv || !a->r || !a->t || !a->d_rays_o || !a->d_rays_d ||
        !a->grad_r || !a->grad_t)
        return -1;
    if (a->n_cams <= 0 || a->cam < 0 || a->cam >= a->n_cams || a->n_samples <= 0) return -2;
    if (a->d_z_out && (a->O <= 0 || !a->z_out)) return -3;
    if (a->n_importance == 0 && a->d_z && (a->N <= 0 || !a->lin_samples)) return -4;
    if (!a->scratch) return -5;
    const int waves = kPoseThreads / 64;
    hipLaunchKernelGGL(pose_ray_terms_kernel, dim3((a->B + waves - 1) / waves), dim3(kPoseThreads), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(pose_adjoint_kernel, dim3(1), dim3(kPoseThreads), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
