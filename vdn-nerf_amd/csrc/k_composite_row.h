// The per-ray compositor (reference dpt_models/renderer.py:262-315): NeuS alpha from (sdf, normal), inside / outside blend with
// the background pass, exclusive transmittance scan, weighted colour sums, eikonal partial sums - one 64-lane wavefront per ray,
// T = N + n_outside <= 256 samples, lane l owns samples 4l .. 4l+3. The VDN feature channels are not its business: their weighted
// sums are a streaming launch of their own (feat_composite_kernel, rays.hip), built on the feature blend below.
//
// One body, three callers: composite_kernel (rays.hip) and composite_train_kernel (train_rays.hip) read sdf / normals / colours of
// the ray from HBM; the fused shading kernel (k_sdf_fwd2.h MODE 2, k_shade_f32.h) gets them from the workgroup that evaluated the
// ray's 128 points, in LDS. The bodies carry `#pragma clang fp contract(off)` like k_ray_rows.h, so every caller rounds like
// rays.hip's -ffp-contract=off build. Also here, because both the forward and the adjoint (train_rays.hip) need them: the feature
// blend and the argument checks of the compositor's entry points.
#pragma once
#include "k_ray_rows.h"

namespace vdn {

// per-sample inputs of the compositor: q = r * N + i (global sample id), i = sample of the ray
struct CompositeGlobalSrc {
    const float* sdf_;
    const float* normals_;
    const float* color_;
    VDN_DEV float sdf(long q, int) const { return sdf_[q]; }
    VDN_DEV float normal(long q, int, int k) const { return normals_[q * 3 + k]; }
    VDN_DEV float color(long q, int, int k) const { return color_[q * 3 + k]; }
};
// the ray's samples in LDS: [7][N] floats = sdf | normal x, y, z | colour r, g, b
struct CompositeLdsSrc {
    const float* rows;
    int n;
    VDN_DEV float sdf(long, int i) const { return rows[i]; }
    VDN_DEV float normal(long, int i, int k) const { return rows[(1 + k) * n + i]; }
    VDN_DEV float color(long, int i, int k) const { return rows[(4 + k) * n + i]; }
};

// what a caller may need in registers: the ray's eikonal partial sums (what eik_partial[2r], [2r+1] receive) and its composited
// colour incl. the background term (what color_out[3r ..] receives); uniform over the wave
struct RowOut { float num, den, c[3]; };
typedef RowOut EikPair;

// eik_partial may be NULL (the fused kernel publishes the returned pair itself). a.feat_out is not looked at.
template <class Src>
VDN_DEV RowOut composite_row(const CompositeArgs& a, int r, int lane, const Src& src) {
#pragma clang fp contract(off)
    const int N = a.N, T = a.T;
    const bool has_bg = a.bg_density != nullptr;
    float o[3], d[3];
    load_ray(a.rays_o, a.rays_d, r, o, d);
    float inv_s = expf(a.variance[0] * 10.0f);                     // fields.py:364
    inv_s = fminf(fmaxf(inv_s, 1e-6f), 1e6f);                      // renderer.py:262
    const float car = a.cos_anneal_dev != nullptr ? a.cos_anneal_dev[0] : a.cos_anneal_ratio;      // (device scalar: graph-captured launches)

    float alpha[kEPL], f[kEPL], Tr[kEPL], wgt[kEPL], col[kEPL][3];
    double eik_num = 0.0, eik_den = 0.0;
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        const int i = kEPL * lane + e;
        alpha[e] = 0.0f;
        f[e] = 1.0f;
        col[e][0] = col[e][1] = col[e][2] = 0.0f;
        if (i < T) {
            float bg_a = 0.0f;
            if (has_bg) {
                const long q = (long)r * T + i;
                bg_a = 1.0f - expf(-softplus1(a.bg_density[q]) * a.bg_dists[q]);   // renderer.py:124
            }
            if (i < N) {
                const long q = (long)r * N + i;
                const float sdf = src.sdf(q, i), dist = a.dists[q];
                const float g0 = src.normal(q, i, 0), g1 = src.normal(q, i, 1), g2 = src.normal(q, i, 2);
                const float true_cos = d[0] * g0 + d[1] * g1 + d[2] * g2;
                const float iter_cos = -(fmaxf(-true_cos * 0.5f + 0.5f, 0.0f) * (1.0f - car) + fmaxf(-true_cos, 0.0f) * car);
                const float est_next = sdf + iter_cos * dist * 0.5f;
                const float est_prev = sdf - iter_cos * dist * 0.5f;
                const float prev_cdf = sigmoidf_(est_prev * inv_s);
                const float next_cdf = sigmoidf_(est_next * inv_s);
                float al = ((prev_cdf - next_cdf) + 1e-5f) / (prev_cdf + 1e-5f);
                al = fminf(fmaxf(al, 0.0f), 1.0f);
                const float pn = sample_norm(o, d, a.mid_z[q]);
                const float inside = pn < 1.0f ? 1.0f : 0.0f;
                eikonal_add(pn, g0, g1, g2, eik_num, eik_den);
                a.cdf[q] = prev_cdf;
                a.inside_sphere[q] = inside;
                // where inside = 0 the blend multiplies the colour head's output by an exact zero: the slot is not read (the head
                // need not have written it; its outputs are sigmoid / ReLU values, so c * 0 is +0 like the 0 that stands in)
                const bool heads = !has_bg || pn < 1.0f;
                float c0 = heads ? src.color(q, i, 0) : 0.0f, c1 = heads ? src.color(q, i, 1) : 0.0f, c2 = heads ? src.color(q, i, 2) : 0.0f;
                if (has_bg) {
                    const long qb = (long)r * T + i;
                    al = al * inside + bg_a * (1.0f - inside);                     // renderer.py:290
                    c0 = c0 * inside + a.bg_rgb[qb * 3] * (1.0f - inside);
                    c1 = c1 * inside + a.bg_rgb[qb * 3 + 1] * (1.0f - inside);
                    c2 = c2 * inside + a.bg_rgb[qb * 3 + 2] * (1.0f - inside);
                }
                alpha[e] = al;
                col[e][0] = c0; col[e][1] = c1; col[e][2] = c2;
            } else {
                const long qb = (long)r * T + i;
                alpha[e] = bg_a;
                col[e][0] = a.bg_rgb[qb * 3]; col[e][1] = a.bg_rgb[qb * 3 + 1]; col[e][2] = a.bg_rgb[qb * 3 + 2];
            }
            f[e] = 1.0f - alpha[e] + 1e-7f;
        }
    }
    ray_excl_cumprod(f, Tr, lane);
    double ws = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
    float wmax = 0.0f;
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        const int i = kEPL * lane + e;
        wgt[e] = 0.0f;
        if (i < T) {
            wgt[e] = alpha[e] * Tr[e];
            a.weights[(long)r * T + i] = wgt[e];
            if (a.alpha_out != nullptr) a.alpha_out[(long)r * T + i] = alpha[e];
            ws += (double)wgt[e];
            c0 += (double)(col[e][0] * wgt[e]);
            c1 += (double)(col[e][1] * wgt[e]);
            c2 += (double)(col[e][2] * wgt[e]);
            wmax = fmaxf(wmax, wgt[e]);
        }
    }
    const float wsum = (float)wave_sum(ws);
    float cr = (float)wave_sum(c0), cg = (float)wave_sum(c1), cb = (float)wave_sum(c2);
    wmax = wave_max(wmax);
    eik_num = wave_sum(eik_num);
    eik_den = wave_sum(eik_den);
    if (a.background_rgb != nullptr) {                                              // renderer.py:309-310
        cr = cr + a.background_rgb[0] * (1.0f - wsum);
        cg = cg + a.background_rgb[1] * (1.0f - wsum);
        cb = cb + a.background_rgb[2] * (1.0f - wsum);
    }
    if (lane == 0) {
        a.color_out[r * 3] = cr; a.color_out[r * 3 + 1] = cg; a.color_out[r * 3 + 2] = cb;
        a.weight_sum[r] = wsum;
        a.weight_max[r] = wmax;
        if (a.s_val != nullptr) a.s_val[r] = 1.0f / inv_s;
        if (a.eik_partial != nullptr) {
            a.eik_partial[r * 2] = (float)eik_num;
            a.eik_partial[r * 2 + 1] = (float)eik_den;
        }
    }
    return RowOut{(float)eik_num, (float)eik_den, {cr, cg, cb}};
}

// ------------------------------------------------------------------------------------------
// The VDN feature channels of a sample, lanes over channels (this lane: ch0 and ch1), blended with the background pass like the
// colour (renderer.py:297-298). A = CompositeArgs or CompositeBwdArgs (same field names).
// ------------------------------------------------------------------------------------------
struct FeatRaw { float fg[2], bg[2]; };      // what memory holds for the two channels: foreground / background feature (0 where absent)
struct FeatPair { float f0, f1; };
// inside: as feat_mix; where the blend gives the foreground feature weight 0 it is not read (+0 stands in: see composite_row)
template <class A>
VDN_DEV FeatRaw feat_load(const A& a, int r, int i, int ch0, int ch1, float inside) {
    const int N = a.N, T = a.T, C = a.feat_ch;
    const bool v0 = ch0 < C, v1 = ch1 < C;
    const bool fg = i < N && (a.bg_density == nullptr || inside != 0.0f), bg = i < T && (a.bg_density != nullptr || i >= N) && a.bg_feat != nullptr;
    const long qf = ((long)r * N + i) * C, qb = ((long)r * T + i) * C;
    FeatRaw v;
    v.fg[0] = (fg && v0) ? a.feat[qf + ch0] : 0.0f;
    v.fg[1] = (fg && v1) ? a.feat[qf + ch1] : 0.0f;
    v.bg[0] = (bg && v0) ? a.bg_feat[qb + ch0] : 0.0f;
    v.bg[1] = (bg && v1) ? a.bg_feat[qb + ch1] : 0.0f;
    return v;
}
// inside: the sample's inside-sphere flag (1 / 0; only looked at for i < N with a background pass)
template <class A>
VDN_DEV FeatPair feat_mix(const A& a, int i, const FeatRaw& v, float inside) {
#pragma clang fp contract(off)
    if (i >= a.N) return FeatPair{v.bg[0], v.bg[1]};
    if (a.bg_density == nullptr) return FeatPair{v.fg[0], v.fg[1]};
    return FeatPair{v.fg[0] * inside + v.bg[0] * (1.0f - inside), v.fg[1] * inside + v.bg[1] * (1.0f - inside)};
}
// blended feature pair of sample i
template <class A>
VDN_DEV FeatPair feat_pair(const A& a, int r, int i, int ch0, int ch1, float inside) {
    return feat_mix(a, i, feat_load(a, r, i, ch0, ch1, inside), inside);
}
// ... of the 8 samples i0 .. i0+7 (those below i_end; zero behind), all 32 loads of the group issued before the first use: a plain
// loop waits out one memory round trip per sample (160 us for 160 samples x 96 channels inside the per-ray kernel)
template <class A>
VDN_DEV void feat_group(const A& a, int r, int i0, int i_end, int ch0, int ch1, const float (&inside)[8], FeatPair (&f)[8]) {
    FeatRaw v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = i0 + k < i_end ? feat_load(a, r, i0 + k, ch0, ch1, inside[k]) : FeatRaw{};
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = i0 + k < i_end ? feat_mix(a, i0 + k, v[k], inside[k]) : FeatPair{};
}

// ------------------------------------------------------------------------------------------
// Argument errors of the compositor's entry points (host side; include/vdn_render.h lists the codes): -1 sizes, -2 inputs,
// -3 outputs, -4 background pass, -5 feature channels; the entry points add what is theirs behind these.
// ------------------------------------------------------------------------------------------
// bwd_bg_ok: the fused forward + adjoint launch also needs the adjoint's background outputs
inline int composite_fwd_check(const VdnCompositeArgs* a, bool need_alpha_out, bool need_eik_out, bool bwd_bg_ok = true) {
    if (!a || a->B <= 0 || a->N <= 0 || a->T < a->N || a->T > kMaxT) return -1;
    if (!a->rays_o || !a->rays_d || !a->sdf || !a->normals || !a->dists || !a->mid_z || !a->color || !a->variance) return -2;
    if (!a->weights || (need_alpha_out && !a->alpha_out) || !a->cdf || !a->inside_sphere || !a->color_out || !a->weight_sum ||
        !a->weight_max || !a->eik_partial || (need_eik_out && !a->eik_out)) return -3;
    if (a->T > a->N && (!a->bg_density || !a->bg_rgb || !a->bg_dists || !bwd_bg_ok)) return -4;
    return 0;
}
// what the feature channels' launch needs besides feat_out
inline bool composite_feat_ok(const VdnCompositeArgs* a) { return a->feat && a->feat_ch > 0 && !(a->T > a->N && !a->bg_feat); }
inline int composite_bwd_check(const VdnCompositeBwdArgs* a, bool need_eik) {
    if (!a || a->B <= 0 || a->N <= 0 || a->T < a->N || a->T > kMaxT) return -1;
    if (!a->rays_o || !a->rays_d || !a->sdf || !a->normals || !a->dists || !a->mid_z || !a->color || !a->variance ||
        !a->alpha || !a->weights || (need_eik && !a->eik)) return -2;
    if (!a->d_sdf || !a->d_normals || !a->d_color || !a->d_var_partial) return -3;
    if (a->T > a->N && (!a->bg_density || !a->bg_rgb || !a->bg_dists || !a->d_bg_density || !a->d_bg_rgb)) return -4;
    if (a->d_feat && (!a->feat || a->feat_ch <= 0 || a->feat_ch > 128)) return -5;
    return 0;
}

}  // namespace vdn
