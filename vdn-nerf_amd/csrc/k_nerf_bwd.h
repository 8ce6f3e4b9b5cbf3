// Backward of the background NeRF MLP on gfx950, shared body for both policies: delta chain through
// the transposed layers with ReLU masks from the saved activations. Adjoint of fields.py:324-353.
// EXPL (standalone NeRF.forward under autograd): the inputs are the given pts4 [P,4] / dirs [P,3] (NerfInputGradArgs)
// instead of points regenerated from rays, and their adjoints d_pts4 / d_dirs are written as they are - no map back
// through the inverted-sphere parameterisation.
#pragma once
#include <type_traits>
#include "mlp_engine.h"
#include "vdn_kernels.h"

namespace vdn {

// MASK (bf16, not EXPL): the ReLU' of the chain comes from the forward's 1-bit masks (a.mask / mask_v; mlp_engine.h:
// BF16::relu_bits) instead of the saved planes save_h / save_hv, which this kernel then does not read
template <class P, bool DPT, bool EXPL, bool MASK = false>
__global__ __launch_bounds__(P::kWaves * 64, P::kMinWavesPerEU) void nerf_bwd_kernel(NerfBwdArgs a, NerfInputGradArgs in) {
    using ST = typename P::store_t;
    constexpr int kSlot = P::stride(9);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WStream<P::kWaves, kSlot> ws;
    const bool want_pts = EXPL || a.d_pts != nullptr;      // input adjoints: three more chunks (W0^T) and the encodings' adjoints
    ws.init(a.blob, smem, want_pts ? 83 : 80);
    const int lane = ws.lane, c = lane & 31, h = lane >> 5;
    // p = row in the (possibly compacted) work list = row of the saves and deltas; pd = dense point id of the upstream grads
    const long n_rows = a.active_idx != nullptr ? (long)*a.n_active : (long)a.P;
    if ((long)blockIdx.x * P::kWaves * 32 >= n_rows) return;
    ws.warm_issue((n_rows + P::kWaves * 32 - 1) / (P::kWaves * 32), 256 * P::kMinWavesPerEU);      // (mlp_engine.h)
    warm_code_issue((std::is_same<P, BF16>::value) ? kWarmCodeNerfBwd : 0, (n_rows + P::kWaves * 32 - 1) / (P::kWaves * 32), 256 * P::kMinWavesPerEU, ws.warm_dump());      // (the kernel's own code: vdn_common.h)
    const long p_raw = ((long)blockIdx.x * P::kWaves + ws.wave) * 32 + c;
    const bool ok = p_raw < n_rows;
    const long p = ok ? p_raw : n_rows - 1;
    const long pd = a.active_idx != nullptr ? (long)a.active_idx[p] : p;
    const long PS = P::plane(a.P, 256);
    constexpr int KO = DPT ? 4 : 1;
    constexpr int LDO = DPT ? 128 : 32;
    const ST* save_h = reinterpret_cast<const ST*>(a.save_h);
    const ST* save_hv = reinterpret_cast<const ST*>(a.save_hv);
    ST* delta_o = reinterpret_cast<ST*>(a.delta_o);
    ST* delta_v = reinterpret_cast<ST*>(a.delta_v);
    ST* delta_head = reinterpret_cast<ST*>(a.delta_head);
    ST* delta_h = reinterpret_cast<ST*>(a.delta_h);
    // MASK: the nine layers' masks (34 VGPRs, where the plane path keeps its prefetched H tiles) are loaded here, ahead of
    // everything else; they land under the weight stream's warm-up wait (mask_landed below). Words 4 l .. 4 l + 3: pts_linears.l;
    // 32, 33: views_linears.0
    unsigned mk[MASK ? 34 : 1];
    if constexpr (MASK) {
        const unsigned char* m = static_cast<const unsigned char*>(a.mask);
        const long MS = BF16::mask_plane(a.P, 256);
#pragma unroll
        for (int l = 0; l < 8; ++l) BF16::load_mask<4>(m + l * MS, p, h, mk + 4 * l);
        BF16::load_mask<2>(static_cast<const unsigned char*>(a.mask_v), p, h, mk + 32);
    }

    // inverted-sphere point and view direction of this lane's sample, as the forward builds them (renderer.py:112-115)
    float x4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dir[3] = {0.0f, 0.0f, 0.0f}, pw[3] = {0.0f, 0.0f, 0.0f}, nrm = 1.0f;
    float dx4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ddir[3] = {0.0f, 0.0f, 0.0f};
    if (EXPL) {
#pragma unroll
        for (int d = 0; d < 4; ++d) x4[d] = in.pts4[pd * 4 + d];
#pragma unroll
        for (int d = 0; d < 3; ++d) dir[d] = in.dirs[pd * 3 + d];
    } else if (want_pts) {
        const long r = pd / a.n_per_ray;
        const float z = a.z[pd];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            dir[d] = a.rays_d[r * 3 + d];
            pw[d] = a.rays_o[r * 3 + d] + dir[d] * z;
        }
        nrm = sqrtf(pw[0] * pw[0] + pw[1] * pw[1] + pw[2] * pw[2]);
        const float rr = fminf(fmaxf(nrm, 1.0f), 1e10f);
#pragma unroll
        for (int d = 0; d < 3; ++d) x4[d] = pw[d] / rr;
        x4[3] = 1.0f / rr;
    }
    typename P::template Act<9> X;
    typename P::template Act<8> Y;
    {   // delta of [rgb (tile 0, rows 0..2) | dpt (tiles 1..3)]: no activation on these heads
        float g3[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) g3[d] = a.g_rgb[pd * 3 + d];
        const f32x16 t16 = vals_tile<3>(g3, h, 0);
        X.set(0, t16);
        P::store_tile(delta_o, p, LDO, 0, h, t16, ok);
        if constexpr (DPT) {
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) {
                const f32x16 g = F32::load_tile(a.g_feat, pd, 96, kt, h);
                X.set(kt + 1, g);
                P::store_tile(delta_o, p, LDO, kt + 1, h, g, ok);
            }
        }
    }
    auto ldH = [&](int l) VDN_INL { return [=](int nt) VDN_INL { return P::load_tile(save_h + l * PS, p, 256, nt, h); }; };
    auto mask_store = [&](auto& D, ST* dst, int ld) VDN_INL {
        return [&D, dst, ld, p, ok, h](int nt, const f32x16& acc, const f32x16& hv) VDN_INL {
            f32x16 o;
#pragma unroll
            for (int t = 0; t < 16; ++t) o[t] = hv[t] > 0.0f ? acc[t] : 0.0f;
            D.set(nt, o);
            P::store_tile(dst, p, ld, nt, h, o, ok);
        };
    };
    // D = acc * mask bit (MASK): the same select, no plane loads. w0: the layer's first mask word
    auto bit_store = [&](auto& D, ST* dst, int ld, int w0) VDN_INL {
        return [&D, &mk, dst, ld, w0, p, ok, h](int nt, const f32x16& acc, int) VDN_INL {
            const f32x16 o = BF16::mask_select(mk + w0, nt, acc);
            D.set(nt, o);
            P::store_tile(dst, p, ld, nt, h, o, ok);
        };
    };
    // pts_linears.l's delta: the layer from `In` (KT k-tiles) into `D`
    auto hidden = [&](auto kt_c, auto& In, auto& D, int l) VDN_INL {
        constexpr int KT = decltype(kt_c)::value;
        if constexpr (MASK) dense<P, KT, 8, false>(ws, In, 0, NoPre{}, bit_store(D, delta_h + l * PS, 256, 4 * l), P::kTileOps);
        else dense<P, KT, 8, false, kBwdPrefetch>(ws, In, 0, ldH(l), mask_store(D, delta_h + l * PS, 256), P::kTileOps, P::kTileOps);
    };
    using K8 = std::integral_constant<int, 8>;
    ws.all_issue = __any(ok);
    if constexpr (MASK) BF16::mask_landed(mk);
    warm_l2_wait();
    ws.start();
    // Wout^T: -> d hv (128), masked by the views layer's ReLU
    if constexpr (MASK) dense<P, KO, 4, false>(ws, X, 0, NoPre{}, bit_store(Y, delta_v, 128, 32), P::kTileOps);
    else dense<P, KO, 4, false>(ws, X, 0, [&](int nt) VDN_INL { return P::load_tile(save_hv, p, 128, nt, h); },
                                    mask_store(Y, delta_v, 128), 4);
    // Wviews^T: -> d [feature (8 tiles) | PE(view) (only wanted for differentiable rays)]; feature_linear has no activation
    dense<P, 4, 9, false>(ws, Y, 0, NoPre{}, [&](int nt, const f32x16& acc, int) VDN_INL {
        if (nt < 8) {
            X.set(nt, acc);
            P::store_tile(delta_head, p, 288, nt, h, acc, ok);
        } else if (want_pts) {
            pe_adjoint_tile<3, 4, 0, P::kAccurateTrig>(acc, h, dir, ddir);
        }
    });
    {   // head delta = [d feature (256) | d density at row 256]
        float g1[1] = {a.g_density[pd]};
        const f32x16 t16 = vals_tile<1>(g1, h, 0);
        X.set(8, t16);
        P::store_tile(delta_head, p, 288, 8, h, t16, ok);
    }
    hidden(std::integral_constant<int, 9>{}, X, Y, 7);     // Whead^T
    hidden(K8{}, Y, X, 6);                                  // W7^T
    hidden(K8{}, X, Y, 5);                                  // W6^T
    // W5^T: 11 output tiles = [PE (3, dropped) | h4 (8)]
    dense<P, 8, 11, false>(ws, Y, 0,
        [&](int nt) VDN_INL {
            if constexpr (MASK) return 0;
            else return nt >= 3 ? P::load_tile(save_h + 4 * PS, p, 256, nt - 3, h) : f32x16{};
        },
        [&](int nt, const f32x16& acc, const auto& hv) VDN_INL {
            if (nt >= 3) {
                f32x16 o;
                if constexpr (MASK) {
                    o = BF16::mask_select(mk + 16, nt - 3, acc);
                } else {
#pragma unroll
                    for (int t = 0; t < 16; ++t) o[t] = hv[t] > 0.0f ? acc[t] : 0.0f;
                }
                X.set(nt - 3, o);
                P::store_tile(delta_h + 4 * PS, p, 256, nt - 3, h, o, ok);
            } else if (want_pts) {          // the skip input's adjoint: slots 32 nt .. of the 10-octave encoding of pts4
                if (nt == 0) pe_adjoint_tile<4, 10, 0, P::kAccurateTrig>(acc, h, x4, dx4);
                else if (nt == 1) pe_adjoint_tile<4, 10, 1, P::kAccurateTrig>(acc, h, x4, dx4);
                else pe_adjoint_tile<4, 10, 2, P::kAccurateTrig>(acc, h, x4, dx4);
            }
        });
    hidden(K8{}, X, Y, 3);      // W4^T
    hidden(K8{}, Y, X, 2);      // W3^T
    hidden(K8{}, X, Y, 1);      // W2^T
    hidden(K8{}, Y, X, 0);      // W1^T
    if (want_pts) {
        dense<P, 8, 3, false>(ws, X, 0, NoPre{}, [&](int nt, const f32x16& acc, int) VDN_INL {       // W0^T
            if (nt == 0) pe_adjoint_tile<4, 10, 0, P::kAccurateTrig>(acc, h, x4, dx4);
            else if (nt == 1) pe_adjoint_tile<4, 10, 1, P::kAccurateTrig>(acc, h, x4, dx4);
            else pe_adjoint_tile<4, 10, 2, P::kAccurateTrig>(acc, h, x4, dx4);
        });
        if (EXPL) {
            if (ok && h == 0) {
#pragma unroll
                for (int d = 0; d < 4; ++d) in.d_pts4[pd * 4 + d] = (in.accumulate ? in.d_pts4[pd * 4 + d] : 0.0f) + dx4[d];
#pragma unroll
                for (int d = 0; d < 3; ++d) in.d_dirs[pd * 3 + d] = (in.accumulate ? in.d_dirs[pd * 3 + d] : 0.0f) + ddir[d];
            }
            return;
        }
        // pts4 = [p / r, 1 / r], r = clip(|p|, 1, 1e10): inside the clip r = |p| (d r / d p = p / r), outside it is a constant
        if (ok && h == 0) {
            const bool free_r = nrm >= 1.0f && nrm <= 1e10f;
            const float rr = fminf(fmaxf(nrm, 1.0f), 1e10f);
            const float pu = pw[0] * dx4[0] + pw[1] * dx4[1] + pw[2] * dx4[2];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float v = dx4[d] / rr;
                if (free_r) v -= pw[d] * (pu / (rr * rr * rr) + dx4[3] / (rr * rr * rr));
                a.d_pts[pd * 3 + d] = v;
                a.d_dirs[pd * 3 + d] = ddir[d];
            }
        }
    }
}

template <class P, bool EXPL>
int launch_nerf_bwd_impl(const VdnNerfBwdArgs* args, const NerfInputGradArgs& in, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int ppw = P::kWaves * 32;
    const int grid = (args->P + ppw - 1) / ppw;
    const size_t lds = 3 * P::stride(9);
    if (args->mask != nullptr || args->mask_v != nullptr) {
        if constexpr (std::is_same<P, BF16>::value && !EXPL) {
            if (args->mask == nullptr || args->mask_v == nullptr) return -5;
            static bool once_m = (allow_big_lds(nerf_bwd_kernel<P, false, false, true>, lds), allow_big_lds(nerf_bwd_kernel<P, true, false, true>, lds), true);
            (void)once_m;
            if (args->g_feat != nullptr)
                hipLaunchKernelGGL((nerf_bwd_kernel<P, true, false, true>), dim3(grid), dim3(P::kWaves * 64), lds, stream, *args, in);
            else
                hipLaunchKernelGGL((nerf_bwd_kernel<P, false, false, true>), dim3(grid), dim3(P::kWaves * 64), lds, stream, *args, in);
            return (int)hipGetLastError();
        } else {
            return -5;          // ReLU masks: the bf16 ray-regenerated path only
        }
    }
    static bool once = (allow_big_lds(nerf_bwd_kernel<P, false, EXPL>, lds), allow_big_lds(nerf_bwd_kernel<P, true, EXPL>, lds), true);
    (void)once;
    if (args->g_feat != nullptr)
        hipLaunchKernelGGL((nerf_bwd_kernel<P, true, EXPL>), dim3(grid), dim3(P::kWaves * 64), lds, stream, *args, in);
    else
        hipLaunchKernelGGL((nerf_bwd_kernel<P, false, EXPL>), dim3(grid), dim3(P::kWaves * 64), lds, stream, *args, in);
    return (int)hipGetLastError();
}

inline bool nerf_bwd_args_ok(const VdnNerfBwdArgs* args) {
    return args && args->P > 0 && args->blob && args->g_density && args->g_rgb && args->save_h && args->save_hv &&
           args->delta_o && args->delta_v && args->delta_head && args->delta_h;
}

template <class P>
int launch_nerf_bwd(const VdnNerfBwdArgs* args, void* stream) {
    if (!nerf_bwd_args_ok(args)) return -1;
    if (args->d_pts && (!args->d_dirs || !args->rays_o || !args->rays_d || !args->z || args->n_per_ray <= 0)) return -2;
    return launch_nerf_bwd_impl<P, false>(args, NerfInputGradArgs{}, stream);
}

// explicit inputs (vdn_nerf_mlp_bwd_input_*): the ray-regenerated input adjoint of VdnNerfBwdArgs (d_pts) must be off
template <class P>
int launch_nerf_bwd_input(const VdnNerfBwdArgs* args, const VdnNerfInputGradArgs* in, void* stream) {
    if (!nerf_bwd_args_ok(args)) return -1;
    if (!in || !in->pts4 || !in->dirs || !in->d_pts4 || !in->d_dirs) return -2;
    if (args->d_pts || args->d_dirs) return -3;
    return launch_nerf_bwd_impl<P, true>(args, *in, stream);
}

}  // namespace vdn
