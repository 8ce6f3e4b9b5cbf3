// Per-ray device functions of the hierarchical sampler, shared by the per-ray kernels (rays.hip) and the fused
// "SDF pass + merge + up-sample" kernel (k_sdf_fwd0_split.h): one 64-lane wavefront per ray, rows in LDS.
// Reference: dpt_models/renderer.py 147-191 (up_sample) with 44-74 (sample_pdf), 193-207 (cat_z_vals).
//
// Numerics follow the reference's CPU path: ATen's CPU cumprod / cumsum accumulate float32 inputs in double and round every
// prefix to float, so the scans here run in double too, and mul/add pairs round like the reference's separate aten ops:
// every function body carries `#pragma clang fp contract(off)` (rays.hip is also built with -ffp-contract=off), so the
// results do not depend on the flags of the translation unit that includes this header.
#pragma once
#include "vdn_common.h"
#include "vdn_kernels.h"

namespace vdn {

constexpr int kRayWaves = 4;      // rays per workgroup
constexpr int kMaxT = 256;        // max samples per ray handled (4 per lane)
constexpr int kEPL = 4;           // samples per lane: lane l owns samples kEPL*l .. kEPL*l + kEPL-1

// one wave per ray, kRayWaves rays per workgroup: this wave's slot in the workgroup, this lane, the wave's ray; false when the ray
// does not exist (the whole wave then leaves the kernel together; the per-ray kernels use no block-level barrier)
VDN_DEV bool ray_of_wave(int B, int& wave, int& lane, int& r) {
    wave = threadIdx.x >> 6;
    lane = threadIdx.x & 63;
    r = blockIdx.x * kRayWaves + wave;
    return r < B;
}
__host__ __device__ inline int ray_blocks(int B) { return (B + kRayWaves - 1) / kRayWaves; }
// host side: launch n_blocks workgroups of kRayWaves waves / a one-wave-per-ray kernel over B rays
template <class Kernel, class... Args>
inline void launch_ray_blocks(Kernel kernel, int n_blocks, void* stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(kRayWaves * 64), 0, (hipStream_t)stream, args...);
}
template <class Kernel, class... Args>
inline void launch_rays(Kernel kernel, int B, void* stream, Args... args) {
    launch_ray_blocks(kernel, ray_blocks(B), stream, args...);
}

VDN_DEV void load_ray(const float* rays_o, const float* rays_d, int r, float (&o)[3], float (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = rays_o[r * 3 + k];
        d[k] = rays_d[r * 3 + k];
    }
}
// |o + d z|: THE norm every inside / relaxed-sphere test, work list and gate of the renderer compares (against 1, 1.2 or a radius);
// one body, so that all of them round alike
VDN_DEV float sample_norm(const float (&o)[3], const float (&d)[3], float z) {
#pragma clang fp contract(off)
    const float x = o[0] + d[0] * z, y = o[1] + d[1] * z, w = o[2] + d[2] * z;
    return sqrtf(x * x + y * y + w * w);
}
// one sample's share of the eikonal sums (renderer.py:313-315): relax * (|n| - 1)^2 and relax, relax = [|p| < 1.2]; pn = |p|
VDN_DEV void eikonal_add(float pn, float g0, float g1, float g2, double& num, double& den) {
#pragma clang fp contract(off)
    const float relax = pn < 1.2f ? 1.0f : 0.0f;
    const float gn = sqrtf(g0 * g0 + g1 * g1 + g2 * g2) - 1.0f;
    num += (double)(relax * (gn * gn));
    den += (double)relax;
}

VDN_DEV double wave_incl_scan_mul(double v, int lane) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(v, off);
        if (lane >= off) v *= t;
    }
    return v;
}
VDN_DEV double wave_incl_scan_add(double v, int lane) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}
VDN_DEV double wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
VDN_DEV float wave_max(float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// exclusive product scan over a ray: in f[e] (lane owns elements kEPL*lane+e), out T[e] = prod_{k<i} f_k
// rounded to float per element (what alpha * cumprod([1, f...])[:-1] multiplies with).
VDN_DEV void ray_excl_cumprod(const float (&f)[kEPL], float (&T)[kEPL], int lane) {
#pragma clang fp contract(off)
    double loc = 1.0;
#pragma unroll
    for (int e = 0; e < kEPL; ++e) loc *= (double)f[e];
    const double incl = wave_incl_scan_mul(loc, lane);
    double run = __shfl_up(incl, 1);
    if (lane == 0) run = 1.0;
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        T[e] = (float)run;
        run *= (double)f[e];
    }
}
// exclusive suffix sums over a ray: S[e] = sum_{k>i} v_k (the compositor's adjoint: sum_{j>i} dL/dw_j w_j)
VDN_DEV void ray_excl_suffix_sum(const double (&v)[kEPL], double (&S)[kEPL], int lane) {
#pragma clang fp contract(off)
    double loc = 0.0;
#pragma unroll
    for (int e = 0; e < kEPL; ++e) loc += v[e];
    double incl = loc;                       // inclusive suffix over lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_down(incl, off);
        if (lane + off < 64) incl += t;
    }
    double run = __shfl_down(incl, 1);       // sum over higher lanes
    if (lane == 63) run = 0.0;
#pragma unroll
    for (int e = kEPL - 1; e >= 0; --e) {
        S[e] = run;
        run += v[e];
    }
}

// ------------------------------------------------------------------------------------------
// one up-sampling round: z[M], sdf[M] -> n_imp new z per ray  (renderer.py:147-191, 44-74)
// ------------------------------------------------------------------------------------------
// the round itself, on a ray whose z / sdf rows (M entries) sit in LDS; cdf: M floats of scratch
VDN_DEV void upsample_row(const UpsampleArgs& a, int r, int lane, int M, const float* z, const float* sd, float* cdf) {
#pragma clang fp contract(off)
    const bool given_w = a.weights != nullptr;
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    if (!given_w) load_ray(a.rays_o, a.rays_d, r, o, d);
    float alpha[kEPL], f[kEPL], T[kEPL];
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        const int i = kEPL * lane + e;
        alpha[e] = 0.0f;
        f[e] = 1.0f;
        if (i < M - 1) {
            const float z0 = z[i], z1 = z[i + 1], s0 = sd[i], s1 = sd[i + 1];
            const bool inside = (sample_norm(o, d, z0) < 1.0f) | (sample_norm(o, d, z1) < 1.0f);
            const float mid_sdf = (s0 + s1) * 0.5f;
            float cosv = (s1 - s0) / (z1 - z0 + 1e-5f);
            const float prev_cos = (i == 0) ? 0.0f : (s0 - sd[i - 1]) / (z0 - z[i - 1] + 1e-5f);
            cosv = fminf(prev_cos, cosv);
            cosv = fminf(fmaxf(cosv, -1e3f), 0.0f) * (inside ? 1.0f : 0.0f);
            const float dist = z1 - z0;
            const float prev_esti = mid_sdf - cosv * dist * 0.5f;
            const float next_esti = mid_sdf + cosv * dist * 0.5f;
            const float prev_cdf = sigmoidf_(prev_esti * a.inv_s);
            const float next_cdf = sigmoidf_(next_esti * a.inv_s);
            alpha[e] = (prev_cdf - next_cdf + 1e-5f) / (prev_cdf + 1e-5f);
            f[e] = 1.0f - alpha[e] + 1e-7f;
        }
    }
    ray_excl_cumprod(f, T, lane);
    // sample_pdf (det=True)
    float w[kEPL];
    double wsum = 0.0;
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        const int i = kEPL * lane + e;
        w[e] = (i < M - 1) ? ((given_w ? a.weights[(long)r * a.w_ld + i] : alpha[e] * T[e]) + 1e-5f) : 0.0f;
        wsum += (double)w[e];
    }
    const float tot = (float)wave_sum(wsum);
    double loc = 0.0;
    float pdf[kEPL];
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        const int i = kEPL * lane + e;
        pdf[e] = (i < M - 1) ? w[e] / tot : 0.0f;
        loc += (double)pdf[e];
    }
    const double incl = wave_incl_scan_add(loc, lane);
    double run = __shfl_up(incl, 1);
    if (lane == 0) run = 0.0;
    if (lane == 0) cdf[0] = 0.0f;
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        const int i = kEPL * lane + e;
        run += (double)pdf[e];
        if (i < M - 1) cdf[i + 1] = (float)run;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < a.n_imp) {
        const float u = a.u[lane];
        int lo = 0, hi = M;                       // searchsorted(cdf, u, right=True): first idx with cdf[idx] > u
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
        }
        const int below = max(lo - 1, 0), above = min(lo, M - 1);
        float denom = cdf[above] - cdf[below];
        denom = denom < 1e-5f ? 1.0f : denom;
        const float t = (u - cdf[below]) / denom;
        a.new_z[(long)r * a.n_imp + lane] = z[below] + t * (z[above] - z[below]);
    }
}

// ------------------------------------------------------------------------------------------
// merge the new samples into the sorted ray (cat + sort + permuted sdf, renderer.py:197-205)
// also used for z_feed = sort(cat(z_vals, z_vals_outside)) (renderer.py:390-391), sdf pointers NULL
// ------------------------------------------------------------------------------------------
// za / zb: this wave's LDS scratch for the old and the new row; lz / ls (optional): LDS copies of the merged z / sdf rows
// old_src (optional): the old row already in LDS (then a.z is not read); new_sdf_src (optional): this ray's K new sdf values on
// chip (then a.new_sdf is not read)
VDN_DEV void merge_row(const MergeArgs& a, int r, int lane, float* za, float* zb, float* lz, float* ls, const float* old_src = nullptr,
                       const float* new_sdf_src = nullptr) {
#pragma clang fp contract(off)
    const int M = a.M, K = a.K;
    for (int i = lane; i < M; i += 64) za[i] = old_src != nullptr ? old_src[i] : a.z[(long)r * a.ld + i];
    for (int j = lane; j < K; j += 64) zb[j] = a.new_z[(long)r * a.K + j];
    __builtin_amdgcn_wave_barrier();
    const bool has_sdf = a.sdf != nullptr;
    // The old row is sorted in every call render() makes (coarse z, earlier merges), so an old element's rank among the
    // old ones is its index and a new element's is a binary search; an unsorted row (possible through z_vals_inject)
    // takes the counting path. Both give the stable ranks of cat + sort: old elements precede equal new ones.
    bool sorted_here = true;
    for (int i = lane; i + 1 < M; i += 64) sorted_here &= za[i] <= za[i + 1];
    const bool old_sorted = __all(sorted_here);
    float oz[kEPL], os[kEPL];
    int opos[kEPL];
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        const int i = lane + 64 * e;
        opos[e] = -1;
        if (i < M) {
            const float v = za[i];
            int cnt = i;
            if (!old_sorted) {
                cnt = 0;
                for (int k = 0; k < M; ++k) cnt += (za[k] < v) | ((za[k] == v) & (k < i));
            }
            for (int j = 0; j < K; ++j) cnt += zb[j] < v;
            opos[e] = cnt;
            oz[e] = v;
            os[e] = has_sdf ? a.sdf[(long)r * a.ld + i] : 0.0f;
        }
    }
    float nz = 0.0f, ns = 0.0f;
    int npos = -1;
    if (lane < K) {
        const float v = zb[lane];
        int cnt = 0;
        if (old_sorted) {
            int lo = 0, hi = M;                       // first index with za[idx] > v  ==  #(za <= v)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (za[mid] <= v) lo = mid + 1; else hi = mid;
            }
            cnt = lo;
        } else {
            for (int k = 0; k < M; ++k) cnt += za[k] <= v;
        }
        for (int j = 0; j < K; ++j) cnt += (zb[j] < v) | ((zb[j] == v) & (j < lane));
        npos = cnt;
        nz = v;
        ns = has_sdf ? (new_sdf_src != nullptr ? new_sdf_src[lane] : a.new_sdf[(long)r * a.K + lane]) : 0.0f;
    }
    __builtin_amdgcn_wave_barrier();   // all reads of the old row are done before it is overwritten in place
#pragma unroll
    for (int e = 0; e < kEPL; ++e) {
        if (opos[e] >= 0) {
            a.z_out[(long)r * a.ld_out + opos[e]] = oz[e];
            if (has_sdf) a.sdf_out[(long)r * a.ld_out + opos[e]] = os[e];
            if (lz != nullptr) { lz[opos[e]] = oz[e]; ls[opos[e]] = os[e]; }
        }
    }
    if (npos >= 0) {
        a.z_out[(long)r * a.ld_out + npos] = nz;
        if (has_sdf) a.sdf_out[(long)r * a.ld_out + npos] = ns;
        if (lz != nullptr) { lz[npos] = nz; ls[npos] = ns; }
    }
}

// ------------------------------------------------------------------------------------------
// section length and mid-point of sample i of a sorted row z[n] (renderer.py:228-230 and 107-109); the last section is
// sample_dist long
// ------------------------------------------------------------------------------------------
struct Section { float dist, mid; };
VDN_DEV Section section(const float* z, int i, int n, float sample_dist) {
#pragma clang fp contract(off)
    const float z0 = z[i];
    const float dist = (i + 1 < n) ? z[i + 1] - z0 : sample_dist;
    return Section{dist, z0 + dist * 0.5f};
}

// ------------------------------------------------------------------------------------------
// work lists (see include/vdn_render.h): background samples whose NeRF++ output the compositor does not multiply by
// zero, and - for the training step - foreground samples inside the relaxed sphere. The norm test is the compositor's
// own (sample_norm).
// ------------------------------------------------------------------------------------------
struct ActiveJob {
    const float* rays_o;
    const float* rays_d;
    const float* mid_z;     // [B,N]
    int B, N, T;            // T samples listed per ray; samples s >= N are always active (background mode)
    float radius;           // background: active iff !(norm < 1); foreground (T == N): active iff norm < radius
    bool background;
    bool complement;        // foreground only: list what the test rejects
    int32_t* active_idx;
    int32_t* n_active;
    int32_t* ray_counts;
    // two-class foreground list (inner > 0; foreground without complement only): the ids with norm < inner come first, ascending,
    // those with inner <= norm < radius behind them, ascending; n_active[0] stays the total, n_inner[0] = the first class's
    // length, n_inner[1] = that length rounded up to whole 128-row workgroups (capped at the total): the row count of the
    // kernels that only need the first class. ray_counts then holds [2B]: first-class counts, second-class counts.
    float inner;
    int32_t* n_inner;
};

VDN_DEV bool sample_active(const ActiveJob& a, int r, int s, const float (&o)[3], const float (&d)[3]) {
    if (s >= a.N) return true;
    const float pn = sample_norm(o, d, a.mid_z[(long)r * a.N + s]);
    return a.background ? !(pn < 1.0f) : (pn < a.radius) != a.complement;
}

// one ray of a work list. FILL = false: count the ray's active samples into ray_counts[r]; FILL = true: write their ids behind
// those of the rays before (ascending dense order, deterministic), the last ray also the list's length
// ... of a two-class foreground list (ActiveJob::inner). A NaN norm is in neither class.
template <bool FILL>
VDN_DEV void active_list_row_classes(const ActiveJob& a, int r, int lane, const float (&o)[3], const float (&d)[3]) {
    int base0 = 0, base1 = 0, total0 = 0;
    if (FILL) {      // first class: behind the first-class ids of the rays before; second class: behind ALL first-class ids
        int acc0 = 0, acc1 = 0, all0 = 0;
        for (int i = lane; i < a.B; i += 64) {
            const int c0 = a.ray_counts[i];
            all0 += c0;
            if (i < r) { acc0 += c0; acc1 += a.ray_counts[a.B + i]; }
        }
        base0 = (int)wave_sum((double)acc0);
        total0 = (int)wave_sum((double)all0);
        base1 = total0 + (int)wave_sum((double)acc1);
    }
    int n0 = 0, n1 = 0;
    for (int s0 = 0; s0 < a.N; s0 += 64) {
        const int s = s0 + lane;
        const float pn = s < a.N ? sample_norm(o, d, a.mid_z[(long)r * a.N + s]) : 2.0f * a.radius;
        const bool in0 = s < a.N && pn < a.inner, in1 = s < a.N && pn < a.radius && !(pn < a.inner);
        const unsigned long long m0 = __ballot(in0), m1 = __ballot(in1), below = (1ull << lane) - 1ull;
        if (FILL && in0) a.active_idx[base0 + n0 + __popcll(m0 & below)] = r * a.N + s;
        if (FILL && in1) a.active_idx[base1 + n1 + __popcll(m1 & below)] = r * a.N + s;
        n0 += __popcll(m0);
        n1 += __popcll(m1);
    }
    if (lane == 0) {
        if (!FILL) {
            a.ray_counts[r] = n0;
            a.ray_counts[a.B + r] = n1;
        } else if (r == a.B - 1) {
            const int total = base1 + n1;
            a.n_active[0] = total;
            a.n_inner[0] = total0;
            a.n_inner[1] = min(total, (total0 + 127) / 128 * 128);
        }
    }
}

template <bool FILL>
VDN_DEV void active_list_row(const ActiveJob& a, int r, int lane, const float (&o)[3], const float (&d)[3]) {
    if (a.inner > 0.0f) return active_list_row_classes<FILL>(a, r, lane, o, d);
    int base = 0;
    if (FILL) {      // offset of this ray = sum of the counts of the rays before it
        int acc = 0;
        for (int i = lane; i < r; i += 64) acc += a.ray_counts[i];
        base = (int)wave_sum((double)acc);
    }
    int n = 0;
    for (int s0 = 0; s0 < a.T; s0 += 64) {
        const int s = s0 + lane;
        const bool act = s < a.T && sample_active(a, r, s, o, d);
        const unsigned long long m = __ballot(act);
        if (FILL && act) a.active_idx[base + n + __popcll(m & ((1ull << lane) - 1ull))] = r * a.T + s;
        n += __popcll(m);
    }
    if (lane == 0) {
        if (!FILL) a.ray_counts[r] = n;
        else if (r == a.B - 1) a.n_active[0] = base + n;
    }
}

}  // namespace vdn
