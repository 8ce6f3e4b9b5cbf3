/* vdn_render.h - C ABI of libvdn_render.so, the MI355X (gfx950) kernel library behind the
 * drop-in `dpt_models` package (vdn-nerf_amd/dpt_models).
 *
 * The reference (BoifZ/VDN-NeRF) has no FFI layer: its boundary is the Python class API of
 * dpt_models/fields.py and dpt_models/renderer.py. Each entry point below names
 * the reference code it stands in for. All pointers are DEVICE pointers unless marked host;
 * `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream, owns no
 * memory and keeps no global state. Return value: 0 = ok, <0 = argument error, >0 = hipError_t.
 *
 * Layout conventions: all tensors fp32 row-major contiguous. P = number of points, B = rays.
 */
#ifndef VDN_RENDER_H
#define VDN_RENDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDN_ABI_VERSION 28

int vdn_abi_version(void);

/* ---- weight preparation ---------------------------------------------------------------------
 * replaces torch.nn.utils.weight_norm's per-forward recomputation (fields.py:65-66,141-142):
 * W_eff[r,:] = v[r,:] * (g[r] / ||v[r,:]||), materialised once per optimizer step. */
typedef struct {
    const float* g;      /* [rows]      weight_g (or NULL: plain Linear, W_eff = v) */
    const float* v;      /* [rows,cols] weight_v (or Linear.weight) */
    float* w_eff;        /* [rows,cols] out */
    float* inv_norm;     /* [rows] out: 1/||v_r|| (kept for the backward), may be NULL */
    int32_t rows, cols;
} VdnWeightNormDesc;
int vdn_weightnorm_materialize(const VdnWeightNormDesc* descs_dev, int n_layers, int max_rows, void* stream);

/* One 32-row MFMA weight chunk to build (see csrc/mlp_engine.h for the chunk format).
 * value(i, k) = scale * src[nmap[n0+i]*row_stride + kmap[k]*col_stride]   (0 where a map entry is -1)
 * so a transposed image is just swapped strides. */
typedef struct {
    const float* src;        /* effective weight matrix */
    const float* bias;       /* [src rows] or NULL */
    const int32_t* kmap;     /* [k_pad] source column per padded input index, -1 = zero */
    const int32_t* nmap;     /* [>= n0+32] source row per padded output index, -1 = zero */
    char* dst;               /* chunk destination inside the blob */
    int64_t row_stride, col_stride;
    int32_t n0;              /* first padded output row of this chunk */
    int32_t k_pad;           /* padded input width of the whole chunk (multiple of 32) */
    float scale;
    int32_t fmt;             /* 0 = fp32 chunk, 1 = bf16 chunk */
    int32_t kt_begin;        /* this descriptor fills k-tiles [kt_begin, kt_begin+kt_count) of the chunk; */
    int32_t kt_count;        /* kmap is indexed from the start of that range. kt_count 0 = whole chunk    */
    int32_t write_bias;      /* 1: also write the chunk's bias/pad block (exactly one descriptor per chunk) */
    float bias_scale;        /* the bias block holds bias_scale * bias[row] */
    const float* tail;       /* optional: tail_n floats copied to dst + tail_off (behind the bias block, inside the chunk's   */
    int32_t tail_off;        /* stride): a small constant that rides along with every chunk's DMA - the bf16 SDF streams carry */
    int32_t tail_n;          /* row 0 of the last layer's weight there (csrc/k_sdf_fwd2.h)                                    */
    int32_t tail_stride;     /* distance between consecutive tail floats in `tail` (0 or 1: contiguous; the colour head's "c2" */
                             /* stream carries one COLUMN of its first layer: stride = that matrix's row length)               */
} VdnChunkDesc;
int vdn_build_images(const VdnChunkDesc* descs_dev, int n_chunks, void* stream);

/* ---- positional encoding as a stand-alone op: embedder.py:27-36 (Embedder.embed) ----------------------------
 * out[p, :] = [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), cos(2^1 x), ...]  (each function over all d inputs, then the next),
 * x = in[p, 0:d]; n_freqs octaves, frequencies 2^k exactly (embedder.py:23). The MLP kernels evaluate the same encoding
 * in registers; this entry point serves callers of embed_fn (e.g. sdf_network.embed_fn_fine). */
int vdn_posenc(const float* in, float* out, int64_t P, int32_t d, int32_t n_freqs, void* stream);

/* ---- SDF network: fields.py:72-108 (SDFNetwork.forward / .sdf / .gradient) --------------------
 * mode 0: sdf only (fields.py:91-92; used by the sampler renderer.py:370,201 and the mesh lattice
 *         renderer.py:441-446).  mode 1: sdf + 256-d feature + analytic d sdf/d x. */
typedef struct {
    const char* blob;          /* weight chunk stream for this mode */
    const float* pts;          /* [P,3], or NULL to generate pts = rays_o[r] + rays_d[r]*z[p], r = p / n_per_ray */
    const float* rays_o;       /* [B,3] */
    const float* rays_d;       /* [B,3] */
    const float* z;            /* [B,z_ld], first n_per_ray columns used */
    int32_t n_per_ray;
    int32_t z_ld;              /* row stride of z (>= n_per_ray) */
    int32_t sdf_ld;            /* row stride of the sdf output, point (r,s) -> sdf[r*sdf_ld+s] (= n_per_ray when dense) */
    int32_t P;                 /* B * n_per_ray (or number of explicit points) */
    float scale;               /* SDFNetwork(scale=...) */
    float* sdf;                /* out, see sdf_ld */
    void* feat;               /* [P,256] out (mode 1) */
    float* normals;            /* [P,3] out (mode 1) */
    void* S;                  /* [8,P,256] workspace: softplus'(pre-activation) per hidden layer (mode 1, f32 entry point).
                               * The bf16 entry point never touches it: it keeps softplus' on the chip (8-bit, LDS + registers) */
    const float* w8row;        /* [256] row 0 of the last layer's effective weight (f32 entry point, mode 1; the bf16 streams carry it) */
    /* training-mode saves (mode 1), optional (H == NULL = nothing saved; with H, V is required and PE optional).
     * The f32 entry point saves in the network's own units. The bf16 entry point saves all three in units of
     * 1/(100 log2 e) (H = 100 log2(e) softplus(a), V = 100 log2(e) v, PE = 100 log2(e) encoding): the units its
     * hidden layers compute in (csrc/k_sdf_fwd2.h). Consumers: s_from_h = 2 in the backward chains, and a factor
     * 1/(100 log2 e) in the finalize scale of the weight-gradient entries that contract over these planes. */
    void* H;                  /* [8,P,256] H[l] = softplus output of layer l (= input of layer l+1) */
    void* V;                  /* [8,P,256] V[l] = sweep value v_l = u_{l+1} * softplus'(a_l) */
    void* PE;                 /* [P,64] positional encoding of the point (39 valid) */
    /* bf16 entry points: every bf16 plane is stored round-to-nearest-even (v_cvt_pk_bf16_f32).
     * Accuracy contract of their encodings (here, in the normals, in the heads' and the background network's view / point
     * encodings): sine and cosine are the hardware instructions on the float32 argument in revolutions
     * (vdn-nerf_amd/csrc/vdn_common.h: sincos_pe), each within 2^-18 + 2^-23 |arg| of the exact function of the exact argument
     * (absolute) - far below the bf16 rounding the encoded value then receives. The f32 entry points use the library sincosf.
     * tests/test_gpu_mlp_planes.py holds the planes to it. */
    /* f32 entry points (here, the heads, the background network and their backward chains; tests/test_gpu_mlp_planes_f32.py holds
     * every plane to it): every plane is row-major f32 [P, ld] in the network's own units (work list: compact rows). Encodings use
     * the library sincosf on the float32 argument 2^k x (x = scale * p rounded once), each value within 1 ulp (2^-23 |y|).
     * An MFMA layer (v_mfma_f32_32x32x2_f32) accumulates in ONE k-ordered chain: the bias first, then for g ascending and
     * j = 0..3 the two products k = 8g+j and k = 8g+4+j of one instruction. How that instruction rounds its two products internally
     * the instruction set manual does not state; this library's ASSUMPTION is a chain of fused multiply-adds, k = 8g+j before
     * k = 8g+4+j, one rounding per product and no wider accumulator - the tests take their float32 floor from that chain
     * (oracle/mlp_ops.py: mfma_chain_f32) and three times the floor absorbs the other readings.
     * H[l] = softplus(100 a_l) / 100 and S[l] = sigmoid(100 a_l), a_l = W_l H[l-1] + b_l, both from one exponential:
     * t = 100 log2(e) a, e = 2^-|t|, u = 1 + e, H = log2(u) ln 2 / 100 + max(a, 0), r = 1 / u, S = a >= 0 ? r : e r (v_exp_f32,
     * v_log_f32, v_rcp_f32: 1 ulp each). A pre-activation of exactly 0 gives S = 1/2 and H = float32(ln 2 / 100) exactly. The
     * hardware exponential may flush a result below 2^-126 to zero: an S below 2^-125 is held to 2^-126 absolute.
     * Layer 3 has 217 outputs: columns 217..223 of H[3] / S[3] / V[3] hold softplus(0), 1/2 and 0 (zero weights, zero bias) and
     * columns 224..255 are never written; neither is promised. */
    /* optional work list (vdn_foreground_active; same contract as VdnNerfArgs.active_idx): per-point inputs / outputs
     * are addressed by the dense point id, training saves and deltas by the compact row */
    const int32_t* active_idx;
    const int32_t* n_active;
    /* optional (mode 1): d sdf / d(encoded input) in the network's own units, the 39 values u with
     * normal = scale * J_PE(x)^T u (fields.py:97-108) - what the ray adjoint needs for the explicit x-dependence of
     * J_PE (learnable poses, poses.py:198-208). Rows follow the saves (compact with a work list). */
    float* U_pe;               /* [P,39] or NULL */
    /* optional (bf16 entry points, mode 1 with a work list): the TAIL of the list. The 128-row kernel runs whole rounds of 256
     * workgroups (one per CU); when the list ends within tail_max_rows rows behind tail_row0 (a multiple of 128, normally one
     * full round = 32 768), vdn_sdf_mlp_fwd_bf16 leaves the rows from tail_row0 on alone and vdn_sdf_fwd_tail_bf16 - called with
     * the SAME struct - evaluates them with 32-row workgroups (csrc/k_sdf_fwd1_split.h): same planes, same values, bit for bit.
     * Both decide on the device-side row count, so both launches are always made. tail_max_rows = 0: off.
     * Promised, with saves and without (tests/test_gpu_sdf_value_launches.py): with n = the list's row count (P without a list),
     * the rows are handed off exactly when tail_row0 < n <= tail_row0 + tail_max_rows. Then vdn_sdf_mlp_fwd_bf16 alone writes rows
     * [0, tail_row0) of every plane and the sdf / normals of their points and nothing else, vdn_sdf_fwd_tail_bf16 alone rows
     * [tail_row0, n) and nothing else, and the two together leave every plane (PE, H, V, feat), sdf and normals as ONE launch with
     * tail_max_rows = 0 does, bit for bit. Otherwise vdn_sdf_mlp_fwd_bf16 evaluates every row and the tail launch writes nothing. */
    int32_t tail_row0, tail_max_rows;
    /* != 0: the launch is part of a training step, where every kernel starts on caches full of other kernels' planes: its first
     * round of workgroups then reads the weight stream into L2 up front (csrc/mlp_engine.h: warm_l2). The launches that save
     * activations do so on their own; a render() loop keeps its weights cached and leaves this 0. */
    int32_t cold_start;
} VdnSdfArgs;
int vdn_sdf_mlp_fwd_f32(int mode, const VdnSdfArgs* args_host, void* stream);
/* bf16-MFMA variant (csrc/k_sdf_fwd2.h): blob holds bf16 chunks (fmt 1) of the SCALED streams (vdn_hip/images.py:
 * sdf_streams(scaled=True): hidden biases x 100 log2 e, last layer's weights / (100 log2 e), sweep weights / 255);
 * feat / H / V / PE are bf16 arrays in the tile-blocked layout of csrc/mlp_engine.h; sdf / normals stay f32.
 * One value per point, whichever launch computes it (tests/test_gpu_sdf_value_launches.py holds each to mode 1 with saves, which
 * tests/test_gpu_mlp_planes.py holds to float64 plane by plane): mode 0 - the feature-split kernel up to 8192 points, the
 * 128-point kernel beyond, on the "sdf" stream, whose layers 0..7 are those of "full" and whose last chunk is its sdf row -
 * returns the sdf of mode 1 BIT FOR BIT (the same operations in the same order: the hidden layers, then the f32 chain over
 * the unrounded activations of layer 7); mode 1 without saves (H = NULL) returns the sdf, normals and feat rows of mode 1 with
 * saves bit for bit; explicit points and the ray form (z_ld, sdf_ld, a work list) alike; cold_start changes no bit. */
int vdn_sdf_mlp_fwd_bf16(int mode, const VdnSdfArgs* args_host, void* stream);
/* mode 1 (+ training saves when H is given) on rows [tail_row0, n) of the work list - see VdnSdfArgs.tail_row0; with
 * tail_row0 = 0 and tail_max_rows >= P it evaluates every row (tests). U_pe must be NULL (-10); tail_max_rows <= 0 or a
 * tail_row0 that is negative or no multiple of 128 is -4; a refused call writes nothing. */
int vdn_sdf_fwd_tail_bf16(const VdnSdfArgs* args_host, void* stream);

/* ---- RenderingNetwork (colour head / 96-channel VDN head): fields.py:148-176, mode 'idr' ------
 * points are regenerated as rays_o[r] + rays_d[r]*z[p] (renderer.py:233), r = p / n_per_ray. */
typedef struct {
    const char* blob;
    const float* rays_o;       /* [B,3] */
    const float* rays_d;       /* [B,3] (also the view direction, renderer.py:234) */
    const float* z;            /* [P] section mid-points */
    const float* normals;      /* [P,3]  d sdf / d x */
    const void* feat;          /* [P,256] SDF feature vector (f32 or bf16, per entry point) */
    const float* pts;          /* [P,3] explicit points (standalone RenderingNetwork.forward) or NULL */
    const float* dirs;         /* [P,3] explicit view dirs or NULL (then rays_d[r]) */
    float* out;                /* [P,d_out] */
    /* bf16 entry point: `out` leaves the last MFMA layer directly - a float32 accumulation of exact bf16 x bf16 products in k-steps
     * of 16 inputs, the accumulator rounded once per k-step: within (number of k-steps) * 2^-24 * sum |w x| of the exact sum over
     * the saved bf16 input plane, through |f'| of the output activation (tests/test_gpu_mlp_planes.py). That the matrix
     * instruction rounds its accumulator once per k-step is this library's ASSUMPTION about v_mfma_f32_32x32x16_bf16 - the
     * instruction set manual does not state its internal rounding -; the bound is what the tests hold the kernels to. */
    void* save_h;              /* [4,P,256] post-ReLU hidden activations (training) or NULL */
    void* save_small;          /* [P,64] the non-feature inputs [points, PE(view), normals] (33 valid) or NULL */
    int32_t n_per_ray;
    int32_t P;
    int32_t d_out;             /* 1..4 or 96 */
    int32_t squeeze_out;       /* 1: sigmoid (fields.py:170-171), 0: relu */
    /* optional work list (vdn_foreground_active; same contract as VdnNerfArgs.active_idx): per-point inputs / outputs
     * are addressed by the dense point id, training saves and deltas by the compact row */
    const int32_t* active_idx;
    const int32_t* n_active;
    /* optional: 96 more feature columns appended to the feature vector - render(depth_before_color=True) feeds the colour
     * network cat([feature_vector, VDN output]) (renderer.py:247-248; a d_feature = 352 network, blob with a 13-k-tile first layer) */
    const float* extra;        /* [P,96] dense point id, or NULL */
    void* save_extra;          /* [P,96] plane of `extra` for the weight-gradient GEMM (training) or NULL */
    /* bf16 training, optional (with save_h): 1-bit ReLU masks of the 4 hidden layers, [4][pad32(P) * 32] bytes
     * (csrc/mlp_engine.h: BF16::relu_bits), for VdnRenderNetBwdArgs.mask; NULL = not written. fp32: must be NULL (-4). */
    void* save_mask;
} VdnRenderNetArgs;
int vdn_rendernet_fwd_f32(const VdnRenderNetArgs* args_host, void* stream);
int vdn_rendernet_fwd_bf16(const VdnRenderNetArgs* args_host, void* stream);   /* bf16-MFMA variant: bf16 chunk blob, bf16 activation workspaces */

/* ---- background NeRF: fields.py:324-353 + the inverted-sphere points of renderer.py:112-115 ---- */
typedef struct {
    const char* blob;
    const float* rays_o;       /* [B,3] */
    const float* rays_d;       /* [B,3] */
    const float* z;            /* [P] mid z of the background pass */
    const float* pts4;         /* [P,4] explicit input_pts (standalone NeRF.forward) or NULL */
    const float* dirs;         /* [P,3] explicit input_views or NULL (then rays_d[r]) */
    float* density;            /* [P] raw alpha_linear output (before softplus) */
    /* bf16 entry point: density, rgb and feat leave their MFMA layer directly and carry the accumulation contract stated at
     * VdnRenderNetArgs.out. */
    float* rgb;                /* [P,3] */
    float* feat;               /* [P,96] dpt_linear output, or NULL when gen_depth_feats is off */
    /* training-mode saves, optional: */
    void* save_h;             /* [8,P,256] post-ReLU outputs of pts_linears.0..7 */
    void* save_pe;            /* [P,96] PE10(pts4) (84 valid) */
    void* save_feature;       /* [P,256] feature_linear output */
    void* save_vpe;           /* [P,32] PE4(view) (27 valid) */
    void* save_hv;            /* [P,128] views_linears.0 output (post-ReLU) */
    int32_t n_per_ray;
    int32_t P;
    /* Optional active-point list (vdn_background_active): only points active_idx[0 .. *n_active) are evaluated; density /
     * rgb / feat are written at their dense positions (the others keep their previous, finite contents - the compositor
     * multiplies them by zero), the training saves are written in COMPACT order (row q holds point active_idx[q]). */
    const int32_t* active_idx; /* [P] or NULL = all points */
    const int32_t* n_active;   /* device scalar */
    /* bf16 training, optional (with save_h, both or neither): 1-bit ReLU masks of pts_linears.0..7, [8][pad32(P) * 32]
     * bytes, and of views_linears.0, [pad32(P) * 16] bytes (csrc/mlp_engine.h: BF16::relu_bits), for VdnNerfBwdArgs.mask /
     * mask_v; NULL = not written. fp32: must be NULL. */
    void* save_mask;
    void* save_mask_v;
} VdnNerfArgs;
int vdn_nerf_mlp_fwd_f32(const VdnNerfArgs* args_host, void* stream);
int vdn_nerf_mlp_fwd_bf16(const VdnNerfArgs* args_host, void* stream);   /* bf16-MFMA variant: bf16 chunk blob, bf16 activation workspaces */

/* ---- per-ray stages of NeuSRenderer (one wavefront per ray) -----------------------------------*/

/* renderer.py:334-359: z = near + (far-near)*linspace(0,1,n) [+ (t_rand-0.5)*2/n];
 * z_out = far / flip(zo) + 1/n, zo = linspace(1e-3, 1-1/(n_out+1), n_out) or its stratified jitter.
 * The linspace vectors are passed in (generated once by the host with torch.linspace so their
 * rounding is the reference's). t_rand / t_rand_out NULL = no perturbation. */
typedef struct {
    const float* near;         /* [B] */
    const float* far;          /* [B] */
    const float* lin_samples;  /* [n_samples] */
    const float* lin_outside;  /* [n_outside] */
    const float* out_lower;    /* [n_outside] */
    const float* out_upper;    /* [n_outside] */
    const float* t_rand;       /* [B] or NULL */
    const float* t_rand_out;   /* [B,n_outside] or NULL */
    float* z;                  /* [B,z_ld] first n_samples columns written */
    float* z_out;              /* [B,n_outside] */
    int32_t B, n_samples, n_outside, z_ld;
} VdnCoarseArgs;
int vdn_coarse_z(const VdnCoarseArgs* args_host, void* stream);

/* renderer.py:147-191 (up_sample) + 44-74 (sample_pdf, det=True) for one round. */
typedef struct {
    const float* rays_o;       /* [B,3] */
    const float* rays_d;       /* [B,3] */
    const float* z;            /* [B,ld] sorted, first M valid */
    const float* sdf;          /* [B,ld] */
    const float* u;            /* [n_imp] = linspace(0.5/n, 1-0.5/n, n) */
    float* new_z;              /* [B,n_imp] */
    float inv_s;               /* 64 * 2^round (renderer.py:378) */
    int32_t B, M, ld, n_imp;
    /* optional: run sample_pdf(bins = z, weights, n_imp, det=True) (renderer.py:44-74) on GIVEN weights instead of the
     * ones up_sample derives from sdf (which, with rays_o / rays_d, may then be NULL) - the form the reference's own
     * sample_pdf vectors are stated in */
    const float* weights;      /* [B,w_ld], first M-1 valid, or NULL */
    int32_t w_ld, _pad;
} VdnUpsampleArgs;
int vdn_upsample_round(const VdnUpsampleArgs* args_host, void* stream);

/* renderer.py:197-205 (cat + sort + sdf permuted alike); also z_feed of renderer.py:390-391 with
 * the sdf pointers NULL. z_out may alias z (in place). */
typedef struct {
    const float* z;            /* [B,ld] first M valid, sorted */
    const float* sdf;          /* [B,ld] or NULL */
    const float* new_z;        /* [B,K] */
    const float* new_sdf;      /* [B,K] or NULL */
    float* z_out;              /* [B,ld_out] first M+K written */
    float* sdf_out;            /* [B,ld_out] or NULL */
    int32_t B, M, K, ld, ld_out;
} VdnMergeArgs;
int vdn_merge_sorted(const VdnMergeArgs* args_host, void* stream);
/* vdn_merge_sorted (with sdf) followed by vdn_upsample_round on the merged rows (M = merge.M + merge.K; the upsample args'
 * z / sdf / ld are ignored: the rows are handed over on chip) - cat_z_vals of round i and up_sample of round i+1
 * (renderer.py:372-386) in one launch. Same results as the two calls. */
int vdn_merge_upsample(const VdnMergeArgs* merge_host, const VdnUpsampleArgs* upsample_host, void* stream);
/* vdn_sdf_mlp_fwd_bf16(mode 0) on the new samples of a round (renderer.py:201; ray form: sdf.z = merge.new_z [B,16],
 * sdf.sdf = merge.new_sdf [B,16]) followed by vdn_merge_upsample on those rays (renderer.py:372-386), in ONE launch: a
 * 32-point workgroup of the small-pass kernel is two rays, whose waves go on to merge and up-sample their rows. Same results
 * as the two calls, bit for bit. Covers 16 new samples per ray, no work list; returns -10 for any other shape (the caller
 * then makes the two calls). */
/* vdn_sdf_mlp_fwd_bf16(mode 0) on the coarse samples (ray form, 64 per ray: renderer.py:369-370) followed by
 * vdn_upsample_round on those rows (upsample.M = 64; its z / sdf / ld are ignored: the rows are handed over on chip), in one
 * launch. Same results as the two calls, bit for bit; -10 for any other shape. */
int vdn_sdf_upsample_bf16(const VdnSdfArgs* sdf_host, const VdnUpsampleArgs* upsample_host, void* stream);
int vdn_sdf_merge_upsample_bf16(const VdnSdfArgs* sdf_host, const VdnMergeArgs* merge_host, const VdnUpsampleArgs* upsample_host, void* stream);

/* renderer.py:228-230 / 107-109: dists = diff(z) with last = sample_dist; mid_z = z + dists/2. */
typedef struct {
    const float* z;            /* [B,ld] */
    float* dists;              /* [B,n] */
    float* mid_z;              /* [B,n] */
    float sample_dist;
    int32_t B, n, ld;
} VdnSectionArgs;
int vdn_sections(const VdnSectionArgs* args_host, void* stream);

/* renderer.py:262-315: NeuS alpha, inside-sphere blend with the background pass, weights =
 * alpha * exclusive-cumprod(1-alpha+1e-7), colour / 96-ch feature sums, eikonal term. */
typedef struct {
    const float* rays_o;       /* [B,3] */
    const float* rays_d;       /* [B,3] */
    const float* sdf;          /* [B*N] */
    const float* normals;      /* [B*N,3] */
    const float* dists;        /* [B,N] */
    const float* mid_z;        /* [B,N] */
    const float* color;        /* [B*N,3] sampled colour */
    const float* feat;         /* [B*N,C] sampled VDN feature or NULL */
    const float* variance;     /* [1] SingleVarianceNetwork.variance (device) */
    const float* bg_density;   /* [B*T] NeRF alpha_linear output, or NULL when n_outside == 0 */
    const float* bg_rgb;       /* [B*T,3] */
    const float* bg_feat;      /* [B*T,C] or NULL */
    const float* bg_dists;     /* [B,T] */
    const float* background_rgb; /* [3] or NULL */
    float cos_anneal_ratio;
    int32_t B, N, T, feat_ch;
    float* weights;            /* [B,T] */
    float* alpha_out;          /* [B,T] blended alpha (kept for the backward) or NULL */
    float* cdf;                /* [B,N] */
    float* inside_sphere;      /* [B,N] */
    float* color_out;          /* [B,3] */
    float* feat_out;           /* [B,C] or NULL */
    float* weight_sum;         /* [B] */
    float* weight_max;         /* [B] */
    float* s_val;              /* [B] 1/inv_s */
    float* eik_partial;        /* [B,2] workspace */
    float* eik_out;            /* [3]: gradient_error, numerator, denominator */
    const float* cos_anneal_dev; /* [1] device scalar or NULL. Non-NULL: the kernels read cos_anneal_ratio from it (the by-value field is
                                  * ignored) - a launch captured once in a HIP graph then follows the runner's annealing schedule
                                  * (dpt_runner.py:304-308) without a re-capture (ABI 28) */
} VdnCompositeArgs;
int vdn_alpha_composite_fwd(const VdnCompositeArgs* args_host, void* stream);
/* d_feats = sum_i w_i * feature_i (renderer.py:306-308) alone, from the `weights` / `inside_sphere` a compositor launch has
 * written: the second launch of vdn_alpha_composite_fwd, for callers whose compositor ran inside vdn_shade_fused_bf16. */
int vdn_feat_composite(const VdnCompositeArgs* args_host, void* stream);

/* ---- renderer.py:239-315 in ONE launch (the north-star kernel; bf16 path, inference): render_core's SDF network + analytic
 * gradient (fields.py:72-108), the colour head (fields.py:148-176, mode 'idr', d_out = 3) and the NeuS alpha / background blend /
 * transmittance scan / weighted sums of vdn_alpha_composite_fwd, for rays of exactly 128 inside samples: one 128-point workgroup
 * evaluates one ray, keeps the 256-d feature vector in registers, runs the colour head on it and composites the ray from LDS; the
 * ray that finishes last reduces the eikonal partial sums of all rays (`ticket`: one int32 arrival counter, zero before the first
 * call; the kernel leaves it zero). sdf: mode-1 arguments in ray form (n_per_ray = 128, P = 128 * comp.B, no work list, no saves;
 * sdf.feat may be NULL - the feature plane is only written when given, for a VDN head launched afterwards); color_blob: the colour
 * network's "c2" stream; comp: as for vdn_alpha_composite_fwd with comp.N = 128 - comp.sdf / normals / color are not read and
 * comp.feat_out must be NULL (the feature channels keep their own launches). Outputs equal the three launches' up to the rounding
 * of the colour head's first layer (the normal's z component enters as an f32 term here, as a bf16 operand there). */
/* renderer.py:239-315 in ONE launch on the exact-fp32 kernels (csrc/k_shade_f32.h; the counterpart of vdn_shade_fused_bf16 on the path
 * that holds the reference's 1e-4): vdn_sdf_mlp_fwd_f32(mode 1) + vdn_rendernet_fwd_f32 (colour head, d_out = 3) +
 * vdn_alpha_composite_fwd + the eikonal reduction, for rays of exactly 128 inside samples (one workgroup per ray), with the very
 * argument blocks of those calls: sdf_host (its sdf / feat / normals / S buffers are required: what passes between the stages goes
 * through them), color_host (feat / normals / z / rays must be sdf_host's, out = the sampled colour [P,3]), comp_host (sdf / normals /
 * color must be those buffers). Same device code as the separate launches: bit-identical outputs. ticket: [1] int32, zero before
 * the first launch. -10 = shape not covered (make the separate calls). */
int vdn_shade_fused_f32(const VdnSdfArgs* sdf_host, const VdnRenderNetArgs* color_host, const VdnCompositeArgs* comp_host,
                        int32_t* ticket, void* stream);
/* The training step's forward of the SDF network and of the colour head in ONE launch (bf16; csrc/k_sdf_fwd2.h MODE 3):
 * vdn_sdf_mlp_fwd_bf16(mode 1) with its training saves (sdf_host->H, V, PE, feat: as there) followed, on the feature vector kept in
 * registers, by vdn_rendernet_fwd_bf16 of the colour network (fields.py:148-176, mode 'idr', d_out = 3) with ITS saves: col_h
 * [4, rows, 256] hidden activations, col_small [rows, 64] the 33 small inputs, col_out [P,3] the colour - the planes
 * VdnRenderNetArgs.save_h / save_small / out name, in the same layouts (compact rows of sdf_host's work list; col_out by dense
 * point id). color_blob: the colour network's "c2" chunk stream (vdn_hip/images.py). One difference from the two launches: the
 * normal's z component enters the first colour layer as an f32 term fmaf(w, nz, acc) on the f32 normal instead of as a bf16
 * operand, so col_h and col_out are not the two launches' bits (col_small is). The contract is stated against the network, not
 * against those launches: col_small = [o + d z (unscaled), PE4(d) of the row's own ray, the f32 normals this launch writes], every
 * col_h[l] is a bf16 rounding of its layer applied to the saved plane before it, col_out the sigmoid layer on col_h[3] in f32 -
 * tests/test_gpu_fused_head_planes.py holds each plane to a float64 model of that layer within max(1, 3 x float32 floor) rounding
 * units (measured: no bf16 plane off the nearest two bf16 values of the model, col_out within 0.17 units). Declines (-10, nothing
 * launched) ray-gradient saves (U_pe) and the tail split (tail_max_rows). */
int vdn_sdf_color_train_bf16(const VdnSdfArgs* sdf_host, const void* color_blob, int32_t squeeze_out, void* col_h, void* col_small,
                             float* col_out, void* stream);
/* ... with a two-class work list (VdnForegroundActiveArgs.n_inner): n_color_rows = n_inner + 1, a device row count of whole
 * 128-row workgroups (or the whole list). Workgroups behind it write no col_h / col_small / col_out - the rows
 * vdn_rendernet_fwd_bf16 leaves alone with that count as its n_active; the SDF side covers the whole list as before. They still
 * run the head's chunk steps (one straight instruction stream per workgroup): the rows are skipped in memory, not in time. */
int vdn_sdf_color_train_rows_bf16(const VdnSdfArgs* sdf_host, const void* color_blob, int32_t squeeze_out, void* col_h, void* col_small,
                                  float* col_out, const int32_t* n_color_rows, void* stream);
int vdn_shade_fused_bf16(const VdnSdfArgs* sdf_host, const void* color_blob, int32_t squeeze_out, const VdnCompositeArgs* comp_host,
                         int32_t* ticket, void* stream);
/* Shading of free-standing points in ONE launch (bf16; csrc/k_sdf_fwd2.h MODE 4) - the vertex attributes of a mesh that goes to
 * disk (vdn_hip/mesh.py: shade_points). Per point x (fp32, object space):
 *     sdf, feat = sdf_network(x);   g = sdf_network.gradient(x)   (raw, not normalised: what render_core feeds the colour head)
 *     view = -g / max(|g|, 1e-12)   (torch.nn.functional.normalize's convention: a zero gradient gives a zero direction, never NaN)
 *     colour = color_network(x, g, view, feat)
 * sdf_host: mode-1 arguments in point form (pts [P,3], any P > 0; sdf [P] and normals [P,3] = g are required outputs; feat is not
 * written and must be NULL); color_blob: the colour network's "c2" stream (mode 'idr', d_feature = 256, d_out = 3); col_out [P,3]:
 * the colour in the network's own channel order. sdf / normals are the bits of vdn_sdf_mlp_fwd_bf16(mode 1). Declines (-10, nothing
 * launched) what it does not cover: training saves (H / V / PE / U_pe), a feature plane, a work list, the tail split. */
int vdn_shade_points_bf16(const VdnSdfArgs* sdf_host, const void* color_blob, int32_t squeeze_out, float* col_out, void* stream);

/* The eikonal sums of renderer.py:313-315 alone - relax_inside_sphere * (|gradient| - 1)^2 and relax_inside_sphere, summed
 * per ray and over the batch, with the compositor's own expressions (same translation unit, bit-identical to the values
 * vdn_alpha_composite_fwd leaves in eik_out) - available as soon as the SDF normals exist: the data-parallel Trainer
 * launches it right behind the fused SDF kernel and all-reduces (numerator, denominator) over the ranks while the colour
 * head, the background network and the compositor still run. */
typedef struct {
    const float* rays_o;       /* [B,3] */
    const float* rays_d;       /* [B,3] */
    const float* mid_z;        /* [B,N] section mid-points */
    const float* normals;      /* [B*N,3] */
    int32_t B, N;
    float* eik_partial;        /* [B,2] workspace */
    float* eik_out;            /* [3]: gradient_error, numerator, denominator */
} VdnEikonalArgs;
int vdn_eikonal_terms(const VdnEikonalArgs* args_host, void* stream);

/* ======================= training step: backward of the render path ============================
 * The reference back-propagates with autograd (dpt_runner.py:253) through renderer.py:209-330 and,
 * twice, through fields.py:97-108. Here the adjoint is hand-derived (DESIGN.md 'Backward'). */

/* backward of RenderingNetwork (fields.py:148-176): delta chain through W^T with ReLU masks from the
 * saved activations; emits per-layer deltas for the weight-gradient GEMM and d feature / d normals. */
typedef struct {
    const char* blob;          /* 'bwd' stream: W4^T, W3^T, W2^T, W1^T, W0^T */
    const float* g_out;        /* [P,d_out] gradient wrt the network output */
    const float* out;          /* [P,d_out] forward output (post sigmoid / relu) */
    const void* save_h;       /* [4,P,256] from the forward */
    void* delta_out;          /* [P,32] (d_out<=4) or [P,96]: delta of the last layer */
    void* delta_h;            /* [4,P,256]: deltas of hidden layers 0..3 */
    void* d_feat;             /* [P,256] d loss / d feature_vector */
    float* d_normals;          /* [P,3] */
    int32_t acc_feat;          /* 0: overwrite d_feat, 1: add into it */
    int32_t acc_normals;       /* 0: overwrite d_normals, 1: add into it */
    int32_t P;
    int32_t d_out;
    int32_t squeeze_out;
    /* optional work list (vdn_foreground_active; same contract as VdnNerfArgs.active_idx): per-point inputs / outputs
     * are addressed by the dense point id, training saves and deltas by the compact row */
    const int32_t* active_idx;
    const int32_t* n_active;
    /* optional input adjoints for differentiable rays (poses.py:198-208): d loss / d points and d loss / d view_dirs
     * (through the 4-octave encoding). dirs / rays_d as in VdnRenderNetArgs (dirs [P,3] or rays_d [B,3] with n_per_ray). */
    const float* dirs; const float* rays_d;
    int32_t n_per_ray;
    int32_t acc_pts;           /* 0: overwrite d_pts / d_dirs, 1: add into them */
    float* d_pts;              /* [P,3] dense point id, or NULL */
    float* d_dirs;             /* [P,3] or NULL */
    /* d_feature = 352 network (VdnRenderNetArgs.extra): d loss / d extra is ADDED into d_extra (the VDN head's output adjoint,
     * which the compositor wrote first) */
    float* d_extra;            /* [P,96] dense point id, or NULL for the 256-feature network */
    /* bf16, optional: the forward's VdnRenderNetArgs.save_mask. Given, the ReLU' of the chain comes from it and save_h is not
     * read (it stays required: the weight-gradient GEMM reads it). fp32: must be NULL (-5). */
    const void* mask;
    /* optional (appended), with a two-class work list (VdnForegroundActiveArgs.n_inner): n_active is then the first class's
     * row count and n_rows_all the whole list's. On the rows [*n_active, *n_rows_all) the output adjoint is exactly zero,
     * so every delta and input adjoint is: with acc_feat = 0 the workgroups there store +0.0 into d_feat (which the SDF
     * backward and its weight-gradient entry read on every listed row) and return - no weight stream, no MFMA; with
     * acc_feat = 1 they return at once (x + 0 = x). d_normals must accumulate (acc_normals = 1) and d_pts must be off (-6). */
    const int32_t* n_rows_all;
} VdnRenderNetBwdArgs;
int vdn_rendernet_bwd_f32(const VdnRenderNetBwdArgs* args_host, void* stream);
int vdn_rendernet_bwd_bf16(const VdnRenderNetBwdArgs* args_host, void* stream);   /* bf16-MFMA variant: bf16 chunk blob, bf16 activation workspaces */

/* backward of the background NeRF (fields.py:324-353). */
typedef struct {
    const char* blob;          /* 'bwd' stream: Wout^T, Wviews^T, Whead^T, W7^T .. W1^T, W0^T (the last only read with d_pts) */
    const float* g_density;    /* [P] */
    const float* g_rgb;        /* [P,3] */
    const float* g_feat;       /* [P,96] or NULL */
    const void* save_h;       /* [8,P,256] */
    const void* save_hv;      /* [P,128] */
    void* delta_o;            /* [P,128] ([P,32] without the dpt head): delta of [rgb | dpt] */
    void* delta_v;            /* [P,128] delta of views_linears.0 */
    void* delta_head;         /* [P,288] delta of [feature_linear (256) | alpha_linear (1)] */
    void* delta_h;            /* [8,P,256] deltas of pts_linears.0..7 */
    int32_t P;
    /* as in VdnNerfArgs: g_* are read at the dense positions, saves and deltas are in compact order */
    const int32_t* active_idx;
    const int32_t* n_active;
    /* optional input adjoints for differentiable rays: with d_pts, the kernel also runs W0^T and maps the adjoints of
     * the two encodings back through pts4 = [p / r, 1 / r], r = clip(|p|, 1, 1e10) (renderer.py:112-115) to
     * d loss / d p and d loss / d view_dir. The points are regenerated from the rays as in VdnNerfArgs. */
    const float* rays_o; const float* rays_d; const float* z;
    int32_t n_per_ray;
    float* d_pts;              /* [P,3] dense point id (rows off the work list are not written), or NULL */
    float* d_dirs;             /* [P,3] (required with d_pts) */
    /* bf16, optional (both or neither): the forward's VdnNerfArgs.save_mask / save_mask_v. Given, the ReLU' of the chain comes
     * from them and save_h / save_hv are not read by this kernel. fp32 and vdn_nerf_mlp_bwd_input_*: must be NULL (-5). */
    const void* mask;
    const void* mask_v;
} VdnNerfBwdArgs;
int vdn_nerf_mlp_bwd_f32(const VdnNerfBwdArgs* args_host, void* stream);
int vdn_nerf_mlp_bwd_bf16(const VdnNerfBwdArgs* args_host, void* stream);   /* bf16-MFMA variant: bf16 chunk blob, bf16 activation workspaces */
/* Input adjoint for EXPLICIT inputs (standalone NeRF.forward under autograd, fields.py:324-353): the forward ran on the given
 * pts4 / dirs (VdnNerfArgs.pts4 / .dirs); the backward of VdnNerfBwdArgs runs as above and also writes d loss / d pts4 and
 * d loss / d dirs as they are (no map back through the inverted-sphere parameterisation). The ray-regenerated adjoint of
 * VdnNerfBwdArgs (d_pts / d_dirs) must be off (-3). Rows are addressed by the dense point id, as g_density. */
typedef struct {
    const float* pts4;         /* [P,4] the forward's input_pts */
    const float* dirs;         /* [P,3] the forward's input_views */
    float* d_pts4;             /* [P,4] out */
    float* d_dirs;             /* [P,3] out */
    int32_t accumulate;        /* 0: overwrite d_pts4 / d_dirs, 1: add into them */
} VdnNerfInputGradArgs;
int vdn_nerf_mlp_bwd_input_f32(const VdnNerfBwdArgs* args_host, const VdnNerfInputGradArgs* in_host, void* stream);
int vdn_nerf_mlp_bwd_input_bf16(const VdnNerfBwdArgs* args_host, const VdnNerfInputGradArgs* in_host, void* stream);

/* backward of SDFNetwork.forward + .gradient (fields.py:72-108), i.e. including the double backward
 * through the input-gradient. Two chains (DESIGN.md 'Backward'):
 *   rbar: adjoint of the reverse sweep, ascending layers, uses the forward weight images;
 *   fbar: adjoint of the forward pass, descending layers, uses the transposed images.
 * Flat workspaces (row-major blocks, P rows each):
 *   UB = [ub0: 64][ub1: 256][ub2: 256][ub3: 256][ub4: 288][ub5: 256][ub6: 256][ub7: 256][ub8: 256]  (2144 cols total)
 *   EX = [8][P][256]   second-order term added to the forward adjoint of each hidden layer
 *   AB = [ab8: 288][ab7: 256] ... [ab0: 256]                                                (2336 cols total) */
typedef struct {
    const char* blob;          /* forward stream of the SDF network (hidden layers 0..7 are used) */
    const float* pts;          /* [P,3] or NULL -> rays */
    const float* rays_o;
    const float* rays_d;
    const float* z;            /* [B,z_ld] */
    int32_t n_per_ray;
    int32_t z_ld;
    int32_t P;
    float scale;
    const float* g_normals;    /* [P,3] d loss / d (d sdf/d x) */
    const void* S;            /* [8,P,256] from the forward: softplus' planes, or - with s_from_h - the saved activations H */
    const void* V;            /* [8,P,256] from the forward */
    void* UB;                 /* out, see above */
    void* EX;                 /* out */
    int32_t s_from_h;          /* 1: S points at the H planes; softplus' = 1 - exp(-100 h) is evaluated in the kernel.
                               * 2: H and V are in units of 1/(100 log2 e) (bf16 forward): softplus' = 1 - 2^-H
                               * 0 and 1 are held by tests/test_gpu_mlp_planes_f32.py (no caller passes 1 today), 2 by
                               * tests/test_gpu_mlp_planes.py; acc_pts = 1 of VdnSdfFbarArgs by both. */
    /* optional work list (vdn_foreground_active; same contract as VdnNerfArgs.active_idx): per-point inputs / outputs
     * are addressed by the dense point id, training saves and deltas by the compact row */
    const int32_t* active_idx;
    const int32_t* n_active;
} VdnSdfRbarArgs;
int vdn_sdf_bwd_rbar_f32(const VdnSdfRbarArgs* args_host, void* stream);
int vdn_sdf_bwd_rbar_bf16(const VdnSdfRbarArgs* args_host, void* stream);   /* bf16-MFMA variant: bf16 chunk blob, bf16 activation workspaces */

typedef struct {
    const char* blob;          /* 'fbar' stream: W8^T, W7^T .. W1^T, W0^T (the last only read with d_pts) */
    const float* g_sdf;        /* [P] */
    const void* g_feat;       /* [P,256] */
    const void* S;            /* [8,P,256] softplus' planes, or - with s_from_h - the saved activations H */
    const void* EX;           /* [8,P,256] from rbar */
    void* AB;                 /* out, see above */
    int32_t P;
    float scale;
    int32_t s_from_h;          /* as in VdnSdfRbarArgs */
    /* optional work list (vdn_foreground_active; same contract as VdnNerfArgs.active_idx): per-point inputs / outputs
     * are addressed by the dense point id, training saves and deltas by the compact row */
    const int32_t* active_idx;
    const int32_t* n_active;
    /* optional input adjoint for differentiable rays: d loss / d point through sdf, feature and normal
     * (incl. the explicit x-dependence of the encoding's Jacobian in normal = scale J_PE(x)^T u). Needs the points
     * (pts, or rays + z as in VdnSdfArgs), the upstream g_normals of rbar and U_pe saved by the forward. */
    const float* pts; const float* rays_o; const float* rays_d; const float* z;
    int32_t n_per_ray, z_ld;
    const float* g_normals;    /* [P,3] */
    const float* U_pe;         /* [P,39] */
    int32_t acc_pts;           /* 0: overwrite d_pts, 1: add into it */
    float* d_pts;              /* [P,3] dense point id, or NULL */
} VdnSdfFbarArgs;
int vdn_sdf_bwd_fbar_f32(const VdnSdfFbarArgs* args_host, void* stream);
int vdn_sdf_bwd_fbar_bf16(const VdnSdfFbarArgs* args_host, void* stream);   /* bf16-MFMA variant: bf16 chunk blob, bf16 activation workspaces */
/* Both chains in ONE launch (bf16, no ray gradients: fbar.d_pts must be NULL, else -10): rbar's second-order term ex_l stays
 * in the wave that produced it (csrc/k_sdf_bwd_split.h), rbar.EX / fbar.EX are not touched. UB and AB come out bit-identical to
 * vdn_sdf_bwd_rbar_bf16 followed by vdn_sdf_bwd_fbar_bf16. The two structs must describe the same rows (P, S, s_from_h, work list).
 * Planes are addressed with 32-bit byte offsets: batches whose AB plane (rows x 2336 bf16) would exceed 4 GiB (P > 919 296) are
 * declined with -10 and nothing is launched; callers then run the two kernels. */
int vdn_sdf_bwd_split_bf16(const VdnSdfRbarArgs* rbar_host, const VdnSdfFbarArgs* fbar_host, void* stream);


/* ---- weight gradients: dW[m,n] = sum_p A[p,m] * B[p,n] over one or two (A,B) segments ----------
 * (A = per-layer delta, B = the layer's input; the second segment carries the sweep term of the SDF
 * net). K is split across workgroups; partial slabs are reduced and scattered by vdn_dw_finalize. */
typedef struct {
    const void* A1; const void* B1;       /* [P,lda1], [P,ldb1]  (f32 or bf16, per entry point) */
    const void* A2; const void* B2;       /* second segment or NULL */
    int32_t lda1, ldb1, lda2, ldb2;
    int32_t P;
    int32_t m_tiles, n_tiles;             /* 32-wide column tiles of A (outputs) and B (inputs); n_tiles may be 0 */
    int32_t splits;
    int32_t wg_begin;                     /* prefix sum of vdn_dw_entry_wgs_*(m_tiles, n_tiles, splits) over the list */
    int32_t _pad;
    float* slab;                          /* [splits, m_tiles*32, n_tiles*32] partial products */
    float* colsum;                        /* [splits, m_tiles*32] partial column sums of A1, or NULL */
    const int32_t* P_dev;                 /* optional device scalar: contract over the first min(P, *P_dev) rows only */
} VdnDwDesc;
int vdn_dw_gemm_f32(const VdnDwDesc* descs_dev, int n_desc, int total_wgs, void* stream);
/* bf16 variant: A/B are bf16 planes in the tile-blocked layout of the bf16 chains, rows padded to a multiple of 32 (the
 * kernel reads whole 32-row blocks and zeroes the rows beyond P itself); with two segments `splits` must be even (first
 * half = segment 1). One workgroup contracts one K split of a 256 x 256 output block. */
int vdn_dw_gemm_bf16(const VdnDwDesc* descs_dev, int n_desc, int total_wgs, void* stream);
/* ... with a launch-wide row cap: descriptors [cap_lo, cap_hi) of this launch contract over at most *cap_rows rows, on top of their
 * own P / P_dev. The training engine caps the colour / VDN heads' entries at the rows the heads evaluated
 * (VdnForegroundActiveArgs.n_inner[1]); the descriptor tables stay as they are. */
int vdn_dw_gemm_rows_f32(const VdnDwDesc* descs_dev, int n_desc, int total_wgs, const int32_t* cap_rows, int cap_lo, int cap_hi, void* stream);
int vdn_dw_gemm_rows_bf16(const VdnDwDesc* descs_dev, int n_desc, int total_wgs, const int32_t* cap_rows, int cap_lo, int cap_hi, void* stream);
/* workgroups one descriptor occupies in the launch (the two kernels tile differently); total_wgs = their sum */
int vdn_dw_entry_wgs_f32(int m_tiles, int n_tiles, int splits);
int vdn_dw_entry_wgs_bf16(int m_tiles, int n_tiles, int splits);

/* reduce the K-splits and scatter from image coordinates to the parameter's own layout:
 * target[rmap[i]*t_stride + cmap[j]] (+)= scale * sum_s slab[s,i,j];  btarget[rmap[i]] (+)= bscale * sum_s colsum[s,i] */
typedef struct {
    const float* slab; const float* colsum;
    const int32_t* rmap; const int32_t* cmap;
    float* target; float* btarget;         /* either may be NULL */
    int64_t t_stride;
    int32_t splits, M, N;                  /* M = m_tiles*32, N = n_tiles*32 */
    int32_t accumulate;                    /* 0: '=' (phase 0), 1: '+=' (phase 1) */
    float scale, bscale;
    /* optional second source for ONE target row: target[xrow, cmap[j]] gets  + xscale * sum_s xsum[s, cmap[j]]  on top of the slab
     * sums (the sdf row of the last SDF layer also collects colsum(ub_8), k_sdf_bwd.h) - instead of a '+=' descriptor and
     * a second launch. The sums are indexed by the TARGET column cmap[j] (< xM), not by the image column j, and ride on the slab's
     * column loop: they are applied only where the descriptor has a target and N > 0 (the one user, the lin8 entry, has N = 256) */
    const float* xsum;                     /* [xsplits, xM] or NULL */
    int32_t xsplits, xM, xrow;
    float xscale;
} VdnDwFinalizeDesc;
int vdn_dw_finalize(const VdnDwFinalizeDesc* descs_dev, int n_desc, int max_M, int phase, void* stream);

/* weight-norm backward: dg_r = <dW_r, v_r>/||v_r||;  dv_r = g_r/||v_r|| * (dW_r - <dW_r,v_r>/||v_r||^2 * v_r) */
typedef struct {
    const float* g; const float* v; const float* inv_norm; const float* dw_eff;
    float* dg; float* dv;
    int32_t rows, cols;
} VdnWeightNormBwdDesc;
int vdn_weightnorm_bwd(const VdnWeightNormBwdDesc* descs_dev, int n_layers, int max_rows, void* stream);

/* ---- adjoint of vdn_alpha_composite_fwd (renderer.py:262-315) ---------------------------------- */
typedef struct {
    /* forward inputs */
    const float* rays_o; const float* rays_d;
    const float* sdf; const float* normals; const float* dists; const float* mid_z;
    const float* color; const float* feat; const float* variance;
    const float* bg_density; const float* bg_rgb; const float* bg_feat; const float* bg_dists;
    const float* background_rgb;
    float cos_anneal_ratio;
    int32_t B, N, T, feat_ch;
    /* saved forward results */
    const float* alpha;        /* [B,T] blended alpha */
    const float* weights;      /* [B,T] */
    const float* eik;          /* [3] gradient_error, numerator, denominator */
    /* upstream gradients (any may be NULL = zero) */
    const float* g_color;      /* [B,3] */
    const float* g_feat;       /* [B,C] */
    const float* g_weights;    /* [B,T] */
    const float* g_eik;        /* [1] d loss / d gradient_error */
    const float* g_cdf;        /* [B,N] d loss / d cdf_fine (= prev_cdf, renderer.py:276,322), or NULL */
    /* outputs */
    float* d_sdf;              /* [B*N] */
    float* d_normals;          /* [B*N,3] alpha + eikonal parts */
    float* d_color;            /* [B*N,3] wrt the colour head's output */
    float* d_feat;             /* [B*N,C] wrt the VDN head's output, or NULL */
    float* d_bg_density;       /* [B*T] */
    float* d_bg_rgb;           /* [B*T,3] */
    float* d_bg_feat;          /* [B*T,C] or NULL */
    float* d_var_partial;      /* [B] per-ray d loss / d variance */
    float* d_variance;         /* [1], or NULL: the caller sums d_var_partial itself (e.g. as one more vdn_dw_finalize descriptor) */
    /* optional, for differentiable rays (all three or none): adjoints of the section lengths and of the ray direction
     * inside true_cos = rays_d . normal (renderer.py:265) */
    float* d_dists;            /* [B,N] */
    float* d_bg_dists;         /* [B,T] (NULL without a background) */
    float* d_dir_cos;          /* [B,3] */
    /* optional scratch for the feature channels, [B*(2T+N)] floats: with it the per-sample feature dot products and the outer
     * products d_feat / d_bg_feat run as two streaming launches around the per-ray kernel (which has only 2 waves per CU) */
    float* feat_scratch;
    const float* cos_anneal_dev; /* [1] device scalar or NULL: as VdnCompositeArgs.cos_anneal_dev */
} VdnCompositeBwdArgs;
int vdn_alpha_composite_bwd(const VdnCompositeBwdArgs* args_host, void* stream);

/* Training step, plain configuration (no mask loss, no depth-feature loss, one rank): vdn_alpha_composite_fwd, the colour term's
 * gradient of vdn_loss_fwd_bwd (g_color = sign(color - true_rgb) / (B + 1e-5) * grad_scale, dpt_runner.py:228-229 with mask = 1;
 * written to g_color [B,3] too) and vdn_alpha_composite_bwd in ONE launch, one wavefront per ray. fwd / bwd: the two calls' own
 * argument blocks (bwd.alpha / bwd.weights must be fwd.alpha_out / fwd.weights; bwd.g_color / g_eik / eik are not read); fg_count:
 * device scalar = the eikonal term's global denominator = the number of inside samples within the relaxed sphere (n_active of
 * vdn_foreground_active); igr_weight = d loss / d gradient_error. fwd.eik_out is NOT written: the loss scalars are left to
 * vdn_eikonal_reduce + vdn_loss_fwd_bwd, which may run later on any stream. Adjoints are bit-identical to the three calls'.
 * -10: a configuration it does not cover (feature channels, g_weights, g_cdf, ray adjoints). */
int vdn_composite_train(const VdnCompositeArgs* fwd_host, const VdnCompositeBwdArgs* bwd_host, const float* true_rgb, float* g_color,
                        const int32_t* fg_count, float igr_weight, float grad_scale, void* stream);
/* gradient_error = sum(num) / (sum(den) + 1e-5) from the per-ray partial sums [B,2] -> eik_out [3] (ratio, num, den). */
int vdn_eikonal_reduce(const float* eik_partial, int32_t B, float* eik_out, void* stream);
/* The same idea with the VDN head (womsk_white_wdepth, one rank, no mask), where the 96 feature channels keep their own streaming
 * launches: vdn_composite_fwd_train = the per-ray compositor + the features' weighted sums (vdn_feat_composite), which also write
 * d loss / d render_feats of the depth-feature term (dpt_runner.py:239-243, mask = 1) into g_feats [B,C]; no eikonal reduce.
 * vdn_composite_bwd_train = vdn_alpha_composite_bwd (bwd.g_feat = that g_feats) with the colour term's gradient made from
 * (color_out, true_rgb) and the eikonal denominator from the foreground work list's length, as in vdn_composite_train; bwd.g_color,
 * bwd.g_eik and bwd.eik are not read. Gradients bit-identical to vdn_alpha_composite_fwd + vdn_loss_fwd_bwd + vdn_alpha_composite_bwd;
 * the loss SCALARS stay with vdn_eikonal_reduce + vdn_loss_fwd_bwd, which the caller may run off the critical path. -10: a
 * configuration it does not cover (extra upstream gradients, ray adjoints). */
int vdn_composite_fwd_train(const VdnCompositeArgs* fwd_host, const float* gt_feats, float* g_feats, float depth_weight, float grad_scale, void* stream);
int vdn_composite_bwd_train(const VdnCompositeBwdArgs* bwd_host, const float* color_out, const float* true_rgb, float* g_color,
                            const int32_t* fg_count, float igr_weight, float grad_scale, void* stream);

/* ---- adjoint of the ray geometry of render_core / render_core_outside (renderer.py:107-115, 228-237): collects the
 * per-point input adjoints of the networks and the section-length adjoints of the compositor into
 * d loss / d rays_o, d rays_d and d loss / d z (inside samples) / d z_out (outside samples), for learnable poses
 * (poses.py:198-208). Geometry: pts = o + d * mid_z, dirs = d; inside: dists_i = z_{i+1} - z_i (last = sample_dist),
 * mid_i = z_i + dists_i / 2; background the same over z_feed = [z | z_out] (every outside sample lies beyond the inside
 * ones, renderer.py:359). One wave per ray. */
typedef struct {
    const float* rays_d;       /* [B,3] */
    const float* mid_z;        /* [B,N] */
    const float* bg_mid;       /* [B,T] or NULL */
    const float* d_pts;        /* [B*N,3] inside points */
    const float* d_dirs;       /* [B*N,3] */
    const float* d_dists;      /* [B,N] */
    const float* d_dir_cos;    /* [B,3] */
    const float* d_bg_pts;     /* [B*T,3] or NULL */
    const float* d_bg_dirs;    /* [B*T,3] */
    const float* d_bg_dists;   /* [B,T] */
    int32_t B, N, T;
    float* d_rays_o;           /* [B,3] */
    float* d_rays_d;           /* [B,3] */
    float* d_z;                /* [B,N] */
    float* d_z_out;            /* [B,T-N] or NULL */
} VdnRayAdjointArgs;
int vdn_ray_adjoint(const VdnRayAdjointArgs* args_host, void* stream);

/* ---- caller semantics of dpt_runner.py:208-243 fused into one launch: loss terms + d loss / d outputs.
 * loss = L1(color)/mask_sum + igr*eik + mask_w*BCE(clip(weight_sum)) + depth_w*L1(feats)/mask_sum.
 * out_scalars = [loss, color_loss, psnr, eikonal, depth_loss, mask_loss]. `grad_scale` multiplies the
 * per-ray gradients (1/world_size under data parallelism). */
typedef struct {
    const float* color;        /* [B,3] */
    const float* true_rgb;     /* [B,3] */
    const float* mask;         /* [B] or NULL (= ones, use_mask False) */
    const float* feats;        /* [B,C] or NULL */
    const float* gt_feats;     /* [B,C] or NULL */
    const float* weights;      /* [B,T] (for weight_sum) */
    const float* eik;          /* [3] gradient_error, num, den */
    float igr_weight, mask_weight, depth_weight, grad_scale;
    int32_t B, T, C, _pad;
    float* g_color;            /* [B,3] */
    float* g_feats;            /* [B,C] or NULL */
    float* g_weights;          /* [B,T] or NULL (only needed when mask_weight != 0) */
    float* g_eik;              /* [1] */
    float* out_scalars;        /* [6] */
} VdnLossArgs;
int vdn_loss_fwd_bwd(const VdnLossArgs* args_host, void* stream);

/* torch.optim.Adam (no weight decay, no amsgrad) over flat buffers: dpt_runner.py:144,254. */
int vdn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, int32_t step, void* stream);
/* The same over the element ranges [begin0, end0) and [begin1, end1) only (the second may be empty), with their own step
 * count: torch.optim.Adam keeps a step per parameter and skips parameters whose grad is None - the VDN head and the
 * background network's dpt_linear until the depth-feature loss switches on (dpt_runner.py:239-243). */
int vdn_adam_step_ranges(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t begin0, int64_t end0,
                         int64_t begin1, int64_t end1, float lr, float beta1, float beta2, float eps, int32_t step, void* stream);

/* ---- on-device ray generator: poses.py:168-212 (fixed poses / intrinsics) + dataset.py:111-118 --------------
 * p = K^-1 [x,y,1]; v = p/|p|; rays_d = R v; rays_o = t; colour / mask / feature gathered from images resident in HBM;
 * near/far from the unit sphere. out row = [rays_o(3) rays_d(3) mask(1) rgb(3) feats(C)] exactly as gen_random_rays_at. */
typedef struct {
    const float* pixels_x;     /* [B] pixel coordinates (already integral-valued for random rays) */
    const float* pixels_y;     /* [B] */
    const float* intrinsic_inv;/* [3,3] row-major (upper-left of the 4x4) */
    const float* pose;         /* [3,4] row-major c2w (upper 3 rows of the 4x4) */
    const float* image;        /* [H,W,3] or NULL */
    const float* mask;         /* [H,W,mask_ch] or NULL (then mask = 1) */
    const float* feats;        /* [H,W,C] or NULL */
    float* out;                /* [B, out_ld] */
    float* near;               /* [B] or NULL */
    float* far;                /* [B] or NULL */
    int32_t B, H, W, C, mask_ch, out_ld;
} VdnGenRaysArgs;
int vdn_gen_rays(const VdnGenRaysArgs* args_host, void* stream);

/* ---- background samples that can reach the image -------------------------------------------------------------------
 * render_core blends the NeRF++ background into the first N (inside) samples with weight (1 - inside_sphere)
 * (renderer.py:284-299): where the section mid-point lies inside the unit sphere the background network's output is
 * multiplied by exactly zero, forward and backward. This kernel lists the other points - sample s < N of ray r is active
 * iff |rays_o + rays_d * mid_z[r,s]| >= 1 (the compositor's own test, same arithmetic), samples s >= N always - in
 * ascending dense order p = r*T + s (deterministic), so the background network can skip the rest without changing one
 * bit of render()'s outputs or gradients. */
typedef struct {
    const float* rays_o;       /* [B,3] */
    const float* rays_d;       /* [B,3] */
    const float* mid_z;        /* [B,N] section mid-points of the inside samples */
    int32_t B, N, T;
    int32_t* active_idx;       /* [B*T] out */
    int32_t* n_active;         /* [1] out */
    int32_t* ray_counts;       /* [B] scratch */
} VdnBackgroundActiveArgs;
int vdn_background_active(const VdnBackgroundActiveArgs* args_host, void* stream);

/* Foreground counterpart, used by the training step only: inside sample s of ray r is active iff
 * |rays_o + rays_d * mid_z[r,s]| < radius. With radius 1.2 the skipped points have inside_sphere = 0 AND
 * relax_inside_sphere = 0 (renderer.py:284-286): their sdf / normal / colour enter the loss only through factors that are
 * exactly zero, so the SDF, colour and VDN networks skip them in the training step (render() itself still evaluates them:
 * it returns `gradients` for every sample). Dense ids p = r*N + s, ascending. */
typedef struct {
    const float* rays_o;
    const float* rays_d;
    const float* mid_z;        /* [B,N] */
    int32_t B, N;
    float radius;
    int32_t complement;        /* nonzero: list the samples the test REJECTS instead (!(|p| < radius)): the two lists of one
                                * (rays, mid_z, radius) partition the B*N samples. render() under grad evaluates the SDF network
                                * with the training saves on the first and without them on the second, which only has to deliver
                                * `gradients` (dpt_models/renderer.py::_RenderCoreFn) */
    int32_t* active_idx;       /* [B*N] out */
    int32_t* n_active;         /* [1] out */
    int32_t* ray_counts;       /* [B] scratch; [2B] with inner_radius */
    /* Two-class list (appended to the struct; both zero: the list above, byte for byte; not with complement). The colour and the VDN head
     * enter the loss only where inside_sphere = 1 (|p| < 1): with inner_radius = 1 the ids with |p| < inner_radius come
     * first (ascending) and those with inner_radius <= |p| < radius behind them (ascending), so compact rows
     * [0, n_inner[0]) are exactly the rows the heads need. n_active[0] stays the total; n_inner[1] = n_inner[0] rounded up
     * to whole 128-row workgroups, capped at the total: the device-side row count of every kernel that runs on the first
     * class only (all of them then touch the same rows). A NaN norm is in neither class. */
    float inner_radius;
    int32_t _pad_inner;
    int32_t* n_inner;          /* [2] out */
} VdnForegroundActiveArgs;

/* The per-ray preparation of a training step in two launches instead of seven: z_feed = sort(cat(z, z_out))
 * (vdn_merge_sorted, renderer.py:390-391), the sections of the inside depths and of z_feed (vdn_sections twice), and both
 * work lists (vdn_foreground_active, vdn_background_active: count pass + fill pass each). Same results element for
 * element. fg_active_idx == NULL skips the foreground list (every inside sample is evaluated: the caller then sets its
 * own row count). */
typedef struct {
    const float* rays_o; const float* rays_d;
    float* z;                  /* [B,z_ld] sorted inside depths; with new_z: the first M_old of them, completed in place */
    const float* new_z;        /* optional [B,N-M_old]: the last up-sampling round's samples, still to be merged into z
                                * (the final cat_z_vals of renderer.py:379-385, which evaluates no sdf), or NULL */
    int32_t M_old, _pad;
    const float* z_out;        /* [B,T-N] outside depths */
    float* z_feed;             /* [B,T] out: sorted [inside | outside] depths */
    int32_t B, N, T, z_ld;
    float sample_dist, fg_radius;
    float* dists; float* mid_z;            /* [B,N] out */
    float* bg_dists; float* bg_mid;        /* [B,T] out */
    int32_t* fg_active_idx; int32_t* fg_n_active; int32_t* fg_ray_counts;     /* as VdnForegroundActiveArgs, or NULL */
    int32_t* bg_active_idx; int32_t* bg_n_active; int32_t* bg_ray_counts;     /* as VdnBackgroundActiveArgs */
    float fg_inner_radius; int32_t _pad_inner; int32_t* fg_n_inner;          /* as VdnForegroundActiveArgs (appended), or zero */
} VdnTrainPrepArgs;
int vdn_train_prep(const VdnTrainPrepArgs* args_host, void* stream);
int vdn_foreground_active(const VdnForegroundActiveArgs* args_host, void* stream);

/* ---- iso-surface of the lattice u = -sdf (device marching tetrahedra) ---------------------------------------------
 * Stands in for mcubes.marching_cubes(u, threshold) of renderer.py:36 (PyMCubes is third-party and not part of the
 * reference tree): every lattice cube is cut into the 6 Kuhn tetrahedra (path 000 -> +e_a -> +e_b -> 111 for the 6
 * axis orders), which is translation invariant, so neighbouring cubes agree on their shared faces and the surface is
 * watertight. "Inside" = u > threshold. Two passes around a prefix sum the caller does:
 *   vdn_mesh_count: counts[cube] = triangles of that cube          (cube = (x*(R-1) + y)*(R-1) + z)
 *   vdn_mesh_emit:  triangle t of a cube -> tri_pos[offset[cube]+t][3 corners][xyz] in lattice index coordinates and
 *                   tri_key[..][3] = a * R^3 + b, the (ordered, a < b) lattice-vertex pair of the cut edge: equal keys
 *                   are the same vertex (bit-identical position), which is how the caller welds the soup.
 * Triangles are wound so that their normal points from inside (u > threshold) to outside. u is [R][R][R] fp32. */
typedef struct {
    const float* u;
    float threshold;
    int32_t R;
    int32_t* counts;           /* [(R-1)^3]   (count pass) */
    const int64_t* offsets;    /* [(R-1)^3] exclusive prefix sum of counts   (emit pass) */
    float* tri_pos;            /* [n_tri][3][3] */
    int64_t* tri_key;          /* [n_tri][3] */
} VdnMeshArgs;
int vdn_mesh_count(const VdnMeshArgs* args_host, void* stream);
int vdn_mesh_emit(const VdnMeshArgs* args_host, void* stream);

/* ---- iso-surface of the lattice as mcubes.marching_cubes(u, threshold) numbers it (renderer.py:36) -------------------------
 * Marching cubes on the classic 256-case tables with PyMCubes' sequential bookkeeping (mcubes/src/marchingcubes.h of
 * PyMCubes 0.1.2, the version the reference's README pins; restated in oracle/marching_cubes.py - the package itself is absent
 * here): cells visited x-major with z innermost, corner "set" when (double)u <= isovalue, one float64 vertex per cut lattice
 * edge created by the first visited cell containing it (in-cell order: edges 6, 5, 10, then 0, 1, 2, 3, 4, 7, 8, 9, 11 where no
 * earlier cell exists), interpolated from the edge's first corner to its second, triangles in table order. Two passes around two
 * exclusive prefix sums over the cells (cell = (x*(R-1) + y)*(R-1) + z) that the caller makes:
 *   vdn_mesh_mc_count: cube_case[cell], n_verts[cell] = vertices the cell creates, n_tris[cell];
 *   vdn_mesh_mc_emit:  vertices[vert_offsets[cell] ..][xyz] (lattice index coordinates) and triangles[tri_offsets[cell] ..][3]
 *                      (vertex numbers) - the arrays the sequential library returns, element for element. u is [R][R][R] fp32. */
typedef struct {
    const float* u;
    double isovalue;
    int32_t R;
    uint8_t* cube_case;            /* [(R-1)^3]   written by the count pass, read by the emit pass */
    int32_t* n_verts;              /* [(R-1)^3]   (count pass) */
    int32_t* n_tris;               /* [(R-1)^3]   (count pass) */
    const int64_t* vert_offsets;   /* [(R-1)^3] exclusive prefix sum of n_verts   (emit pass) */
    const int64_t* tri_offsets;    /* [(R-1)^3] exclusive prefix sum of n_tris    (emit pass) */
    double* vertices;              /* [V][3] */
    int64_t* triangles;            /* [F][3] */
} VdnMeshMcArgs;
int vdn_mesh_mc_count(const VdnMeshMcArgs* args_host, void* stream);
int vdn_mesh_mc_emit(const VdnMeshMcArgs* args_host, void* stream);

/* ---- the same mesh from the cells near the surface only (csrc/mesh_sparse.hip; vdn_hip/mesh.py: marching_cubes_sparse) ---------
 * The (R-1)^3 cells are cut into nb^3 bricks of brick^3 cells, nb = ceil((R-1) / brick), brick number (bi*nb + bj)*nb + bk; the last
 * brick per axis may be partial. The caller chooses the ACTIVE bricks (one field value per brick against a Lipschitz
 * bound), lists them in ascending brick number in `active` [A] and evaluates the field at their nodes only:
 *   vdn_mesh_sparse_nodes: points[p - first][xyz] for first <= p < first + n_points, p = slot * E^3 + (a*E + b)*E + c with
 *                          E = brick + 1: the world coordinates (X[.], Y[.], Z[.]) of lattice node (bi*brick + a, bj*brick + b,
 *                          bk*brick + c) of brick active[slot], each index clamped to R - 1. X, Y, Z are the lattice's three
 *                          coordinate vectors [R], so the floats are the dense lattice's.
 * `values` [A][E][E][E] holds the field at those points. The cells of the active bricks are then triangulated as vdn_mesh_mc_*
 * triangulates the full lattice. The per-cell arrays are COMPACT: a cell's slot is its rank among the active cells in ascending
 * global cell number (i*(R-1) + j)*(R-1) + k - the dense visiting order with the skipped cells left out - so the caller's two
 * exclusive prefix sums over the compact arrays are the dense offsets. The rank of cell (i, j, k) of active brick (bi, bj, bk) is
 *   cell_base[brick] + (i - bi*brick) * row_cells[bi] + (j - bj*brick) * col_cells[bi*nb + bj] + (k - bk*brick)
 * with col_cells[bi][bj] = active cells of one (i, j) column through brick column (bi, bj), row_cells[bi] = active cells of one
 * i-plane through brick layer bi, cell_base = the active cells before the brick's first plane + before its first column in that
 * plane + below it in its own column (the caller's prefix sums over the brick tables). brick_map [nb^3] = slot in `active` or -1.
 *   vdn_mesh_sparse_count: cube_case / n_verts / n_tris at each active cell's rank, and *missed += 1 (the caller zeroes it) for
 *                          every (active cell, cut edge of it, existing cell round that edge that lies in a dropped brick): there
 *                          the surface leaves the evaluated region, i.e. the caller's bound does not hold.
 *   vdn_mesh_sparse_emit:  vertices and triangles as vdn_mesh_mc_emit writes them; a triangle corner whose owner cell lies in a
 *                          dropped brick (a missed edge) is left unwritten and nothing is read for it.
 * A rank outside [0, n_cells), a vertex offset outside [0, V) or a triangle offset outside [0, F) is skipped, never dereferenced.
 * Status -10: nb^3, A * (brick+1)^3 (and with it A * brick^3) do not fit 32-bit indexing, or brick > 1024. */
typedef struct {
    const float* X;                /* [R] */
    const float* Y;                /* [R] */
    const float* Z;                /* [R] */
    const int32_t* active;         /* [A] brick numbers, ascending */
    float* points;                 /* [n_points][3] */
    int64_t first, n_points;       /* the range of p this call writes */
    int32_t R, brick, nb, A;
} VdnMeshSparseNodesArgs;
int vdn_mesh_sparse_nodes(const VdnMeshSparseNodesArgs* args_host, void* stream);

typedef struct {
    const float* values;           /* [A][brick+1][brick+1][brick+1] */
    double isovalue;
    int32_t R, brick, nb, A;
    const int32_t* active;         /* [A] */
    const int32_t* brick_map;      /* [nb^3] */
    const int32_t* cell_base;      /* [nb^3]  (read at active bricks only) */
    const int32_t* col_cells;      /* [nb^2] */
    const int32_t* row_cells;      /* [nb] */
    int64_t n_cells;               /* active cells inside the lattice = the length of the compact arrays */
    uint8_t* cube_case;            /* [n_cells]   written by the count pass, read by the emit pass */
    int32_t* n_verts;              /* [n_cells]   (count pass) */
    int32_t* n_tris;               /* [n_cells]   (count pass) */
    int32_t* missed;               /* [1]         (count pass) */
    const int64_t* vert_offsets;   /* [n_cells] exclusive prefix sum of n_verts   (emit pass) */
    const int64_t* tri_offsets;    /* [n_cells] exclusive prefix sum of n_tris    (emit pass) */
    int64_t V, F;                  /* the sums (emit pass) */
    double* vertices;              /* [V][3] */
    int64_t* triangles;            /* [F][3] */
} VdnMeshSparseArgs;
int vdn_mesh_sparse_count(const VdnMeshSparseArgs* args_host, void* stream);
int vdn_mesh_sparse_emit(const VdnMeshSparseArgs* args_host, void* stream);

/* ---- mesh evaluation: area-weighted surface samples of a triangle mesh (csrc/mesh_eval.hip; vdn_hip/mesh.py: sample_surface) ---
 * The sample set an accuracy / completeness / Chamfer figure against a scanned cloud is taken over (vdn_train/mesh_eval.py).
 * Deterministic, no random state. Two passes around an exclusive prefix sum the caller makes:
 *   vdn_surf_count: counts[f] = ceil(area_f / spacing^2), area_f = 0.5 |(b - a) x (c - a)| in double; 0 where the area is 0 or
 *                   not finite (clamped to INT32_MAX). A corner index outside [0, V) gives counts[f] = 0 and sets *error = 1
 *                   (the caller zeroes it first): nothing is read out of bounds.
 *   vdn_surf_emit:  one thread per SAMPLE s < S: its triangle f by binary search in `offsets`, j = s - offsets[f], the R2
 *                   low-discrepancy point (u, v) = frac(0.5 + (j + 1) (0.7548776662466927, 0.5698402909980532)) in double, folded
 *                   into the triangle ((u, v) -> (1 - u, 1 - v) where u + v > 1), points[s] = a + u (b - a) + v (c - a) rounded
 *                   to fp32, face[s] = f.
 * Status -10: V, F or S do not fit 32-bit indexing. */
typedef struct {
    const float* vertices;         /* [V][3] */
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes) */
    double spacing;                /* one sample per spacing^2 of area */
    int64_t V, F, S;               /* S = sum of counts (emit pass) */
    int32_t index_bytes, _pad;     /* 8 or 4 */
    int32_t* counts;               /* [F]   (count pass) */
    int32_t* error;                /* [1]   (count pass) */
    const int64_t* offsets;        /* [F] exclusive prefix sum of counts   (emit pass) */
    float* points;                 /* [S][3] */
    int32_t* face;                 /* [S] */
} VdnSurfArgs;
int vdn_surf_count(const VdnSurfArgs* args_host, void* stream);
int vdn_surf_emit(const VdnSurfArgs* args_host, void* stream);

/* ---- mesh evaluation: exact nearest neighbour on a uniform grid (csrc/mesh_eval.hip; vdn_hip/nn.py: PointGrid) --------------
 * The grid is dense over the reference's bounding box: nx * ny * nz cells of edge h from (lo_x, lo_y, lo_z), cell id
 * (z * ny + y) * nx + x with each coordinate floor((p - lo) / h) in fp32 clamped into the grid (so a point outside the box, or NaN,
 * lands in a border cell).
 *   vdn_nn_bin:   cell[i] of pts[i], i < N. The caller sorts the reference by cell (stable), packs it as 16-byte records
 *                 {x, y, z, original index as bits} in `ref` and makes cell_start[c] = first record of cell c, cell_start[cells] = R.
 *   vdn_nn_query: one lane per query pts[order[t]] (order: the queries' own cell-sorted order, or NULL), Chebyshev shells
 *                 k = 0, 1, .. around the query's cell. With r = k h - margin the search stops after shell k when r > 0 and
 *                 (best <= r or r >= max_dist), or when the shell has left the grid on all sides: every point in a cell at index
 *                 distance >= k + 1 is at least k h away, less the rounding of the fp32 binning, which `margin` (a few ulps of
 *                 the box extent) covers. dist = sqrt(sum (q - r)^2) in fp32, the lower original index on equal distances;
 *                 dist = +inf, idx = -1 where no reference point lies within max_dist (inclusive; +inf: unbounded).
 *                 rings[q] (optional) = shells visited.
 * Status -10: N, R or the cell count do not fit 32-bit indexing. */
typedef struct {
    const float* pts;              /* [N][3] the points to bin / the queries */
    int32_t* cell;                 /* [N] out   (bin) */
    const float* ref;              /* [R][4] sorted packed reference   (query) */
    const int32_t* cell_start;     /* [nx*ny*nz + 1]   (query) */
    const int32_t* order;          /* [N] or NULL   (query) */
    float* dist;                   /* [N] out   (query) */
    int64_t* idx;                  /* [N] out   (query) */
    int32_t* rings;                /* [N] out or NULL   (query) */
    int64_t N, R;
    float lo_x, lo_y, lo_z, h, margin, max_dist;
    int32_t nx, ny, nz, _pad;
} VdnNnArgs;
int vdn_nn_bin(const VdnNnArgs* args_host, void* stream);
int vdn_nn_query(const VdnNnArgs* args_host, void* stream);

/* ---- mesh evaluation: greedy radius thinning of a cloud (csrc/mesh_eval.hip; vdn_hip/nn.py: thin_points) -----------------------
 * One round of the parallel form of "visit the points in index order; a point that is still there removes every other point within
 * `radius` (inclusive)". The cloud is in the sorted 16-byte records and cell_start table of the grid above (vdn_nn_bin's cells,
 * h >= radius + the binning margin, so the 27 cells around a point hold all its neighbours). state[t] belongs to record t:
 * 0 undecided, 1 kept, 2 removed; the caller zeroes it before the first round.
 *   vdn_thin_round: one lane per record. A decided lane does nothing. An undecided one scans the nine (y, z) rows around its cell,
 *                   each as one record range over its three x-cells, for points with a LOWER original index and
 *                   dx^2 + dy^2 + dz^2 <= radius^2 in fp32 (the difference form of vdn_nn_query): one of them kept -> this point is
 *                   removed; all of them removed (or none there) -> kept; otherwise it stays undecided and is counted in
 *                   *undecided (one atomic add per wave; the caller zeroes the word before each round). States are updated in
 *                   place: a decision is final and depends on final decisions only, so reading a neighbour's state late delays a
 *                   decision and never changes it. No lane waits for another. The caller repeats rounds until *undecided == 0;
 *                   every round decides at least the lowest undecided index.
 * Status -10: N or the cell count do not fit 32-bit indexing. */
typedef struct {
    const float* rec;              /* [N][4] sorted packed records {x, y, z, original index as bits} */
    const int32_t* cell_start;     /* [nx*ny*nz + 1] */
    int32_t* state;                /* [N] in / out, per record */
    int32_t* undecided;            /* [1] in / out */
    int64_t N;
    float lo_x, lo_y, lo_z, h, radius;
    int32_t nx, ny, nz;
} VdnThinArgs;
int vdn_thin_round(const VdnThinArgs* args_host, void* stream);

/* ---- mesh cleaning: connected components of a triangle mesh (csrc/mesh_clean.hip; vdn_hip/mesh.py: connected_components) --------
 * Two triangles are connected when they share a vertex INDEX (no welding by position). A lock-free union-find over the index
 * buffer in `parent` [V], which the caller initialises to 0, 1, .., V - 1:
 *   vdn_cc_union:   one thread per triangle joins its three corners. A join finds the two roots and hooks the LARGER root under
 *                   the smaller by a compare-and-swap on the root's own slot; a loser continues from the value the swap returned.
 *                   Slots only ever decrease (the find loop halves long paths by atomic minimum), no thread waits for another.
 *                   A corner index outside [0, V) sets *error = 1 (the caller zeroes it first) and that triangle joins nothing:
 *                   nothing is read or written out of bounds. Degenerate (a, a, b) and repeated triangles are legal.
 *   vdn_cc_flatten: one thread per vertex, label[v] = root of v = the SMALLEST vertex index of v's component: independent of the
 *                   thread order, identical between calls and under any permutation of the triangles. A vertex in no triangle
 *                   is its own component. F = 0 is legal here (label = parent's roots).
 * Status -10: V or F do not fit 32-bit indexing. */
typedef struct {
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes)   (union) */
    int32_t* parent;               /* [V] in / out (union), in (flatten) */
    int32_t* label;                /* [V] out   (flatten) */
    int32_t* error;                /* [1]   (union) */
    int64_t V, F;
    int32_t index_bytes, _pad;     /* 8 or 4 */
} VdnCcArgs;
int vdn_cc_union(const VdnCcArgs* args_host, void* stream);
int vdn_cc_flatten(const VdnCcArgs* args_host, void* stream);

/* vdn_tri_area: area[f] = 0.5 |(b - a) x (c - a)| in double from the fp32 vertices (the expression of vdn_surf_count, one device
 * function for both), 0 where the result is not finite. A corner outside [0, V) gives area 0 and sets *error = 1. */
typedef struct {
    const float* vertices;         /* [V][3] */
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes) */
    double* area;                  /* [F] out */
    int32_t* error;                /* [1] */
    int64_t V, F;
    int32_t index_bytes, _pad;
} VdnTriAreaArgs;
int vdn_tri_area(const VdnTriAreaArgs* args_host, void* stream);

/* ---- mesh cleaning: object masks (csrc/mesh_clean.hip; vdn_hip/mesh.py: dilate_masks, mask_votes) ------------------------------
 * vdn_mask_dilate: dst = the maximum of src over the (2 radius + 1)^2 square around each pixel, pixels outside the image counting
 *   as 0 (cv.dilate with a kernel of ones; nonzero = set, so a 0 / 1 or 0 / 255 mask keeps its two values). Separable: a row pass
 *   src -> scratch and a column pass scratch -> dst, two launches; scratch is a plane set of its own. radius = 0 copies.
 * vdn_mask_votes: one thread per vertex, looping over the N cameras, no atomics. P[n] maps the mesh's own frame to (u w, v w, w),
 *   evaluated in double on the widened fp32 vertex; px = floor(u + 0.5), py = floor(v + 0.5) (pixel centres at integer coordinates,
 *   as vdn_gen_rays has them). The vertex is "in image" of camera n iff w > 0, u and v are finite and 0 <= px < W, 0 <= py < H;
 *   n_in_image[v] counts those cameras, n_in_mask[v] those of them whose mask is nonzero at (py, px).
 * Status -10: V, N * H * W or H * W do not fit 32-bit indexing. */
typedef struct {
    const uint8_t* src;            /* [N][H][W] */
    uint8_t* scratch;              /* [N][H][W] workspace */
    uint8_t* dst;                  /* [N][H][W] out (may be src) */
    int64_t N;
    int32_t H, W, radius, _pad;
} VdnMaskDilateArgs;
int vdn_mask_dilate(const VdnMaskDilateArgs* args_host, void* stream);

typedef struct {
    const float* vertices;         /* [V][3] */
    const double* P;               /* [N][3][4] row-major */
    const uint8_t* masks;          /* [N][H][W] nonzero = set */
    int32_t* n_in_image;           /* [V] out */
    int32_t* n_in_mask;            /* [V] out */
    int64_t V, N;
    int32_t H, W;
} VdnMaskVotesArgs;
int vdn_mask_votes(const VdnMaskVotesArgs* args_host, void* stream);

/* ---- mesh cleaning: face / vertex compaction (csrc/mesh_clean.hip; vdn_hip/mesh.py: filter_mesh) ------------------------------
 * Two passes around the exclusive prefix sums the caller makes:
 *   vdn_mesh_filter_mark:  face_alive[f] = keep_face[f] (or 1 where NULL) and keep_vertex of all three corners (where not NULL);
 *                          a surviving face stores 1 to vertex_used of its corners (the caller zeroes vertex_used first; plain
 *                          byte stores of one value). A corner outside [0, V) kills the face and sets *error = 1.
 *   vdn_mesh_filter_remap: surviving face f goes to row face_offsets[f] of out_triangles, in the input's order and index width,
 *                          each corner i renumbered to vertex_new[i].
 * Status -10: V or F do not fit 32-bit indexing. */
typedef struct {
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes) */
    const uint8_t* keep_face;      /* [F] or NULL   (mark) */
    const uint8_t* keep_vertex;    /* [V] or NULL   (mark) */
    uint8_t* face_alive;           /* [F] out (mark), in (remap) */
    uint8_t* vertex_used;          /* [V] in / out   (mark) */
    int32_t* error;                /* [1]   (mark) */
    const int64_t* face_offsets;   /* [F] exclusive prefix sum of face_alive   (remap) */
    const int64_t* vertex_new;     /* [V] new index of each surviving vertex   (remap) */
    void* out_triangles;           /* [F_out][3]   (remap) */
    int64_t V, F, F_out;           /* F_out = sum of face_alive */
    int32_t index_bytes, _pad;
} VdnMeshFilterArgs;
int vdn_mesh_filter_mark(const VdnMeshFilterArgs* args_host, void* stream);
int vdn_mesh_filter_remap(const VdnMeshFilterArgs* args_host, void* stream);

/* ---- mesh cleaning: ray casting against the mesh on a uniform grid (csrc/mesh_ray.hip; vdn_hip/mesh.py: MeshGrid) ---------------
 * The grid is dense over the bounding box of the referenced, finite vertices: nx * ny * nz cubic cells of edge h from
 * (lo_x, lo_y, lo_z), cell id (z * ny + y) * nx + x, the coordinate of a point floor((p - lo) / h) in double, clamped into the grid.
 * A triangle is REFERENCED unless a corner is not finite, two corner indices are equal or its area (vdn_tri_area's expression) is
 * 0; it is referenced from every cell its axis-aligned box, grown by `margin` on all sides, overlaps. Two passes around the
 * exclusive prefix sum over cells the caller makes:
 *   vdn_ray_bin_count: one thread per triangle: cell_count[c] += 1 (integer atomics; the caller zeroes cell_count first) for each
 *                      overlapped cell, and the triangle's packed record {a, b, c as 9 fp32, the 3 corner indices as int32 bits}
 *                      (zeros for a triangle that is not referenced). A corner index outside [0, V) sets *error = 1 (the caller
 *                      zeroes it first) and the triangle is not referenced: nothing is read or written out of bounds.
 *   vdn_ray_bin_fill:  the same walk; refs[cursor[c]++] = f (integer atomics on `cursor`, which the caller initialises to the
 *                      exclusive prefix sum of cell_count): the order of the references inside a cell is unspecified, and no
 *                      result below depends on it.
 *   vdn_ray_cast:      one lane per ray o + t d, o and d in double. The ray-triangle test is two-sided Moller-Trumbore in double
 *                      on the widened fp32 corners a, b, c, every product and sum rounded on its own (no fused multiply-add), sums
 *                      left to right:
 *                          e1 = b - a, e2 = c - a, p = d x e2 = (d1 e2_2 - d2 e2_1, d2 e2_0 - d0 e2_2, d0 e2_1 - d1 e2_0),
 *                          det = e1_0 p0 + e1_1 p1 + e1_2 p2; no hit when det == 0 or det is not finite; inv = 1 / det,
 *                          s = o - a, u = (s0 p0 + s1 p1 + s2 p2) inv, q = s x e1 (the pattern of p),
 *                          v = (d0 q0 + d1 q1 + d2 q2) inv, t = (e2_0 q0 + e2_1 q1 + e2_2 q2) inv;
 *                          a hit iff u >= 0, v >= 0, u + v <= 1 and t_min < t < t_max (NaN fails every comparison).
 *                      One (ray, triangle) pair therefore gives one t, whichever cell it is found through. Closest hit: the
 *                      smallest t, the lower face index on equal t - independent of the reference order, the thread order and h.
 *                      t[r] = +inf, face[r] = -1 on a miss. any_hit != 0: the walk ends at the first accepted hit; only
 *                      face[r] >= 0 is specified then. skip_vertex[r] (optional): triangles with that corner index are ignored.
 *                      tests[r] (optional) = ray-triangle tests made. Traversal: the segment is clipped to the grid's box grown
 *                      by `margin` (slabs, in double), then a 3-D DDA from the entry cell; the exit parameter of a cell on axis k
 *                      is (lo_k + (i_k + 1 or 0) h - o_k) (1 / d_k), computed from the cell index, not accumulated. After the
 *                      references of a cell are tested the walk ends when the best t <= the cell's exit parameter, when the
 *                      exit parameter reaches the clipped segment's end, or when the next cell is outside the grid; it takes at
 *                      most nx + ny + nz + 3 steps by the loop's own counter. A miss, decided before the loop: an origin or
 *                      direction that is not finite, a direction with no component whose reciprocal is finite (zero), a window
 *                      that is empty or NaN, no overlap with the box. An axis with such a component is never crossed.
 *   vdn_visibility_votes: one lane per (camera n, vertex x), camera-major, integer atomic adds into the two counts (the caller
 *                      zeroes them). "In image" is vdn_mask_votes' rule (one device function for both); a vertex in image of n
 *                      is visible from it iff no triangle without x as a corner is hit by centres[n] + t (x - centres[n]),
 *                      0 < t < 1 - eps (any-hit walk, skip_vertex = x's index).
 * Status -10: V, F, R, n_refs or the cell count do not fit 32-bit indexing. */
typedef struct {
    const float* vertices;         /* [V][3] */
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes) */
    int32_t* cell_count;           /* [nx*ny*nz] in / out   (count) */
    int32_t* cursor;               /* [nx*ny*nz] in / out   (fill) */
    int32_t* refs;                 /* [n_refs] out   (fill) */
    float* records;                /* [F][12] out   (count) */
    int32_t* error;                /* [1]   (count) */
    int64_t V, F, n_refs;          /* n_refs = sum of cell_count   (fill) */
    double lo_x, lo_y, lo_z, h, margin;
    int32_t nx, ny, nz, index_bytes;
} VdnRayGridArgs;
int vdn_ray_bin_count(const VdnRayGridArgs* args_host, void* stream);
int vdn_ray_bin_fill(const VdnRayGridArgs* args_host, void* stream);

typedef struct {
    const double* origins;         /* [R][3] */
    const double* directions;      /* [R][3] */
    const int64_t* skip_vertex;    /* [R] or NULL */
    const float* records;          /* [F][12] */
    const int32_t* cell_start;     /* [nx*ny*nz + 1] */
    const int32_t* refs;           /* [n_refs] */
    double* t;                     /* [R] out */
    int64_t* face;                 /* [R] out */
    int32_t* tests;                /* [R] out or NULL */
    int64_t R, F, n_refs;
    double lo_x, lo_y, lo_z, h, margin, t_min, t_max;
    int32_t nx, ny, nz, any_hit;
} VdnRayCastArgs;
int vdn_ray_cast(const VdnRayCastArgs* args_host, void* stream);

typedef struct {
    const float* vertices;         /* [V][3] */
    const double* P;               /* [N][3][4] row-major */
    const double* centres;         /* [N][3] camera centres, -M^-1 p4 */
    const float* records;          /* [F][12] */
    const int32_t* cell_start;     /* [nx*ny*nz + 1] */
    const int32_t* refs;           /* [n_refs] */
    int32_t* n_in_image;           /* [V] in / out */
    int32_t* n_visible;            /* [V] in / out */
    int64_t V, N, F, n_refs;
    double lo_x, lo_y, lo_z, h, margin, eps;
    int32_t nx, ny, nz, H, W, _pad;
} VdnVisibilityArgs;
int vdn_visibility_votes(const VdnVisibilityArgs* args_host, void* stream);

/* ---- mesh simplification: quadric vertex clustering (csrc/mesh_simplify.hip; vdn_hip/mesh.py: cluster_quadrics, simplify_mesh) ----
 * Rossignac-Borrel cells with Lindstrom's per-cell quadric. The grid has nx * ny * nz cubic cells of edge h; cell (ix, iy, iz) of a
 * point p is floor((double(p) - origin) / h) per axis (a division), the grid covers the cell indices lo_k .. lo_k + n_k - 1, and
 * key = (ix - lo_x) + nx * ((iy - lo_y) + ny * (iz - lo_z)) as int64 (lo = 0 when origin is the box's minimum corner). All arithmetic
 * is double on the widened fp32 vertices, every product and sum rounded on its own (the file is built without contraction). No float
 * atomics: every sum has a fixed order. The sorts, scans and `unique` between the passes are the caller's torch ops.
 *   vdn_simplify_mark:    one thread per triangle. live[f] = 1 iff its three corners are finite; a live triangle stores 1 to
 *                         vertex_used of its corners (the caller zeroes it; plain byte stores of one value). A corner index outside
 *                         [0, V) sets *error = 1 (the caller zeroes it first), the triangle is not live, nothing is touched out of
 *                         bounds.
 *   vdn_simplify_keys:    one thread per vertex: key[v] as above; -1 for a vertex that is not finite or lies outside the grid.
 *   vdn_simplify_records: one thread per triangle. corner_cluster[3 f + c] = vertex_cluster of corner c for a live triangle, else
 *                         the sentinel C (so that a sort by cluster id puts the dead records last); survive[f] = 1 iff the triangle
 *                         is live and its three clusters are pairwise distinct; canonical[f] = the three cluster ids rotated so
 *                         that the smallest comes first (orientation preserved; C, C, C where the triangle does not survive).
 *   vdn_segment_mean:     one wave per segment s: out[s][k] = (sum over j in [start[s], start[s+1]) of rows[members[j]][k]) / count
 *                         in double, generic over K fp32 columns (positions and per-vertex attributes alike); an empty segment gives
 *                         NaN (0 / 0). `members` is the inverted index a stable sort by cluster id gives: ascending vertex index
 *                         inside a segment.
 *   vdn_cluster_quadrics: one wave per cluster over its corner records, `members` = the stable sort of corner_cluster, i.e.
 *                         (triangle, corner) order inside a cluster. Record e = 3 f + c adds triangle f's plane quadric, recomputed
 *                         from the triangle: with pa, pb, pc the corners in the triangle's own order MINUS centre[s],
 *                             n = (pb - pa) x (pc - pa) = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0),
 *                             d = -((n0 pa0 + n1 pa1) + n2 pa2),
 *                             (n0 n0, n0 n1, n0 n2, n1 n1, n1 n2, n2 n2, n0 d, n1 d, n2 d, d d)
 *                         (n unnormalised: area-squared weights; a degenerate triangle adds zeros) -> quadric [C][10] double.
 *   The summation order of both segmented sums: lane l of 64 adds its list's entries j = l, l + 64, l + 128, .. in increasing j,
 *   starting from +0.0; then for s = 32, 16, 8, 4, 2, 1: partial[l] += partial[l + s] for l < s. Bitwise reproducible.
 *   vdn_cluster_place:    one thread per cluster. m = mean[s] (relative to the cell centre), A, b from the quadric,
 *                         tr = (Axx + Ayy) + Azz. tr not positive and finite: x = m, status 1. Otherwise (A + eps tr I) delta =
 *                         -b - A m solved directly in double (cofactors), x = m + delta; x not finite or |x_k| > h / 2 on an axis:
 *                         x = m, status 2. position[s] = centre[s] + x, status[s] as a byte.
 * Status -10: V, F, C or K * the row count do not fit 32-bit indexing. */
typedef struct {
    const float* vertices;         /* [V][3] */
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes) */
    uint8_t* live;                 /* [F] out (mark), in (records) */
    uint8_t* vertex_used;          /* [V] in / out   (mark) */
    int32_t* error;                /* [1]   (mark) */
    int64_t* key;                  /* [V] out   (keys) */
    const int64_t* vertex_cluster; /* [V] cluster id or -1   (records) */
    int64_t* corner_cluster;       /* [3 F] out   (records) */
    int64_t* canonical;            /* [F][3] out   (records) */
    uint8_t* survive;              /* [F] out   (records) */
    int64_t V, F, C;
    double origin_x, origin_y, origin_z, h;
    int64_t lo_x, lo_y, lo_z, nx, ny, nz;
    int32_t index_bytes, _pad;
} VdnSimplifyArgs;
int vdn_simplify_mark(const VdnSimplifyArgs* args_host, void* stream);
int vdn_simplify_keys(const VdnSimplifyArgs* args_host, void* stream);
int vdn_simplify_records(const VdnSimplifyArgs* args_host, void* stream);

typedef struct {
    const float* rows;             /* [N][K] */
    const int64_t* members;        /* [M] row numbers, segment by segment */
    const int64_t* start;          /* [C + 1] ascending, start[C] <= M */
    double* out;                   /* [C][K] */
    int64_t N, M, C;
    int32_t K, _pad;
} VdnSegmentMeanArgs;
int vdn_segment_mean(const VdnSegmentMeanArgs* args_host, void* stream);

typedef struct {
    const float* vertices;         /* [V][3] */
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes); the records' triangles are live: corners in range */
    const int64_t* members;        /* [M] record numbers 3 f + c, cluster by cluster   (quadrics) */
    const int64_t* start;          /* [C + 1]   (quadrics) */
    const double* centre;          /* [C][3] */
    double* quadric;               /* [C][10] out (quadrics), in (place) */
    const double* mean;            /* [C][3] relative to the centre   (place) */
    double* position;              /* [C][3] out   (place) */
    uint8_t* status;               /* [C] out   (place) */
    int64_t V, F, M, C;
    double h, eps;
    int32_t index_bytes, _pad;
} VdnClusterQuadricArgs;
int vdn_cluster_quadrics(const VdnClusterQuadricArgs* args_host, void* stream);
int vdn_cluster_place(const VdnClusterQuadricArgs* args_host, void* stream);

/* ---- adaptive simplification: octree vertex clustering under an error bound (csrc/mesh_simplify.hip; vdn_hip/mesh.py: cluster_octree,
 * select_octree, count_octree_faces, simplify_mesh(tolerance=..); restated in tests/test_mesh_octree_cpu.py) -------------
 * Levels. Level 0 is the clustering above at cell size h0 from `origin`, cells i0 = floor((double(v) - origin) / h0). The level-l
 * cell of a level-0 cell is i0 >> l per axis (an arithmetic shift: floor, also for negative indices), its edge h_l = h0 2^l, its
 * centre origin + (i_l + 0.5) h_l: the cell floor((v - origin) / h_l), since scaling by a power of two is exact. The grid of level l
 * covers lo_l = lo_0 >> l .. hi_l = hi_0 >> l per axis; its cells are numbered in ascending key
 * (ix - lo_x) + nx ((iy - lo_y) + ny (iz - lo_z)), as at level 0. 1 <= levels <= 8.
 * Node record, per level: quadric[10] and mean[3] relative to the node's own centre, count (the referenced vertices in it),
 * position[3] = centre + x, status, error, trace. Level 0 takes quadric and mean from vdn_cluster_quadrics / vdn_segment_mean.
 *   vdn_octree_merge:  one thread per node p of level l. Merge mode (children != NULL): the child in slot s = bx + 2 by + 4 bz is the
 *                      cell 2 i_l + (bx, by, bz) of level l - 1, found by binary search of its key in child_key (ascending);
 *                      children[p][s] = its index, -1 when absent. The present children are taken in ascending s, every sum starting
 *                      from +0.0. With d = (bx ? q : -q, by ? q : -q, bz ? q : -q), q = 0.25 h (the child's centre minus the
 *                      parent's) and (A, b, c), m, n the child's record:
 *                          Ad_i = (A_i0 d0 + A_i1 d1) + A_i2 d2;   A' = A;   b'_i = b_i - Ad_i;
 *                          c' = (c - 2 ((b0 d0 + b1 d1) + b2 d2)) + ((d0 Ad_0 + d1 Ad_1) + d2 Ad_2);
 *                          quadric += (A', b', c');   count += n;   S_i += double(n) (m_i + d_i);
 *                      mean_i = S_i / double(count). Measure mode (children == NULL): quadric and mean are inputs (level 0).
 *                      Then, in both modes, place and measure: x and status are vdn_cluster_place's, by the same device function,
 *                      called with this level's h and eps; with Ax_i = (A_i0 x0 + A_i1 x1) + A_i2 x2,
 *                          e = (((x0 Ax_0 + x1 Ax_1) + x2 Ax_2) + 2 ((b0 x0 + b1 x1) + b2 x2)) + c;   error = e > 0 ? e : 0   (NaN -> 0)
 *                          trace = (Axx + Ayy) + Azz.
 *                      error / trace is the area-squared-weighted mean squared distance from x to the planes of the node's triangles.
 *   vdn_octree_select: one thread per node of a level l >= 1: accept = trace > 0 and trace < inf and error < tolerance2 * trace
 *                      (strict; tolerance2 = tolerance * tolerance, rounded once by the caller); solid = accept and every present
 *                      child's child_solid byte is set. Level 0 is solid by definition (the caller fills ones).
 *   vdn_octree_assign: one thread per level-0 cluster over the level-major concatenation of the levels (node g of level l has the
 *                      global number level_start[l] + g): parent[n] = the global number of n's parent, -1 at the top; while the
 *                      parent is solid, climb (at most `levels` times). Solidity is hereditary downwards, so this is the highest
 *                      solid ancestor. level[c] = its level, node[c] = its number inside that level.
 * All arithmetic is double, every product and sum rounded on its own. Status -10: C, Cc or N beyond 32-bit indexing. */
typedef struct {
    const int64_t* cell;           /* [C][3] this level's cell indices   (merge mode) */
    const double* centre;          /* [C][3] */
    const int64_t* child_key;      /* [Cc] the previous level's keys, ascending   (merge mode) */
    const double* child_quadric;   /* [Cc][10]   (merge mode) */
    const double* child_mean;      /* [Cc][3]   (merge mode) */
    const int64_t* child_count;    /* [Cc]   (merge mode) */
    int64_t* children;             /* [C][8] out, or NULL: measure mode */
    double* quadric;               /* [C][10] out (merge mode), in (measure mode) */
    double* mean;                  /* [C][3] out (merge mode), in (measure mode) */
    int64_t* count;                /* [C] out   (merge mode) */
    double* position;              /* [C][3] out */
    uint8_t* status;               /* [C] out */
    double* error;                 /* [C] out */
    double* trace;                 /* [C] out */
    int64_t C, Cc;
    int64_t lo_x, lo_y, lo_z, nx, ny, nz;   /* the previous level's grid   (merge mode) */
    double h, eps;                 /* this level's edge */
} VdnOctreeMergeArgs;
int vdn_octree_merge(const VdnOctreeMergeArgs* args_host, void* stream);

typedef struct {
    const double* error;           /* [C] */
    const double* trace;           /* [C] */
    const int64_t* children;       /* [C][8] indices into the previous level, -1: absent */
    const uint8_t* child_solid;    /* [Cc] */
    uint8_t* solid;                /* [C] out */
    int64_t C, Cc;
    double tolerance2;
} VdnOctreeSelectArgs;
int vdn_octree_select(const VdnOctreeSelectArgs* args_host, void* stream);

typedef struct {
    const int64_t* parent;         /* [N] global numbers, -1 at the top */
    const uint8_t* solid;          /* [N] */
    const int64_t* level_start;    /* [levels + 2] ascending, level_start[0] = 0, level_start[levels + 1] = N */
    uint8_t* level;                /* [C0] out */
    int64_t* node;                 /* [C0] out */
    int64_t C0, N;
    int32_t levels, _pad;
} VdnOctreeAssignArgs;
int vdn_octree_assign(const VdnOctreeAssignArgs* args_host, void* stream);

/* ---- textured meshes: a per-face atlas baked on the device (csrc/mesh_texture.hip; vdn_hip/mesh.py: texel_points, project_step,
 * gather_atlas, sample_texture, bake_texture) -----------------------------------------------------------------------
 * The atlas is S x S texels, uint8 RGB, row 0 at the top, cut into C x C square cells of n x n texels, C = S / n (integer), n >= 4;
 * the strip right of and below the cells (S % n columns and rows) is unused. Face f owns half h = f & 1 of cell c = f >> 1, whose
 * origin is the texel ((c % C) n, (c / C) n). With m = n - 3 and local texel (i, j) = (column, row) inside the cell:
 *   lower half (h = 0): owns i + j <= n - 2, T = n (n - 1) / 2 texels. Corners 0, 1, 2 of the face sit at the texel centres (0, 0),
 *     (m, 0), (0, m), i.e. at the continuous coordinates (0.5, 0.5), (m + 0.5, 0.5), (0.5, m + 0.5). A texel with i + j <= m has the
 *     barycentrics b1 = i / m, b2 = j / m, b0 = (1 - b1) - b2; a gutter texel, i + j = n - 2, takes the nearest point of the
 *     hypotenuse: b1 = clamp((i - 0.5) / m, 0, 1), b2 = 1 - b1, b0 = 0.
 *   upper half (h = 1): the lower half turned by 180 degrees - local (i, j) is read as (n - 1 - i, n - 1 - j) - so it owns
 *     i + j >= n and its corners sit at (n - 0.5, n - 0.5), (n - 0.5 - m, n - 0.5), (n - 0.5, n - 0.5 - m).
 *   the diagonal i + j = n - 1 belongs to nobody and repeats the texel (i, j - 1), or (i - 1, 0) where j = 0 (both are gutter texels
 *     of the lower half); every other unowned texel - the upper half of a last, half-filled cell, empty cells, the strip - is 0.
 * Texel points are numbered face-major, q = f T + r, r running over j = 0 .. n - 2 (outer), i = 0 .. n - 2 - j (inner) in the
 * half's own (turned) frame: r = j (2 n - 1 - j) / 2 + i. All of it is integer arithmetic, restated in tests/test_mesh_texture_cpu.py.
 *   vdn_tex_points:  one thread per texel point q: points[q] = fp32((b0 v0 + b1 v1) + b2 v2) in double from the double vertices (every
 *                    product and sum rounded on its own: the file is built without contraction), face[q] = f. A corner index outside
 *                    [0, V) sets *error = 1 (the caller zeroes it first) and gives the point (0, 0, 0).
 *   vdn_tex_gather:  one thread per atlas texel, gather form: the texel finds its cell, its half and r (or the diagonal's source, or
 *                    nothing) and writes its three bytes once, rint(clip(c, 0, 1) * 255) in fp32 of colors[q] read in BGR order and
 *                    stored as RGB (vdn_hip.mesh.quantize_colors_bgr). n_colors must equal F T.
 *   vdn_tex_sample:  one thread per query: face[r] in [0, F) and a point. (b1, b2) of the point's projection onto the face's plane
 *                    solve the 2 x 2 normal equations of e1 = v1 - v0, e2 = v2 - v0 against w = p - v0 in double:
 *                      det = a11 a22 - a12 a12;  b1 = (a22 r1 - a12 r2) / det;  b2 = (a11 r2 - a12 r1) / det
 *                    (b1 = b2 = 0 where det is not positive and finite), clamped into the triangle: b1 = max(b1, 0), b2 = max(b2, 0),
 *                    and where s = b1 + b2 > 1 both are divided by s (NaN compares false: such a coordinate becomes 0). Continuous
 *                    atlas coordinates: x = ox + 0.5 + m b1, y = oy + 0.5 + m b2 (lower), x = ox + n - 0.5 - m b1, y = oy + n - 0.5 - m b2
 *                    (upper). Bilinear taps at floor(x - 0.5), floor(y - 0.5) and their successors, indices clamped to [0, S - 1];
 *                    rgb = fp32(((w00 t00 + w10 t10) + (w01 t01 + w11 t11)) / 255) per channel in double. A face outside [0, F)
 *                    (-1 = miss) gives the background; a corner index outside [0, V) sets *error = 1 and gives the background.
 * Inside a face every tap with a non-zero weight is a texel the face owns, so nothing bleeds between faces under
 * bilinear filtering at the base level; mip levels mix neighbours. Status -10: V, F, F T, R or S S beyond 32-bit indexing. */
typedef struct {
    const double* vertices;        /* [V][3]   (points, sample) */
    const void* triangles;         /* [F][3] int64 or int32 (index_bytes)   (points, sample) */
    float* points;                 /* [F T][3] out   (points) */
    int32_t* face;                 /* [F T] out   (points) */
    int32_t* error;                /* [1]   (points, sample) */
    const float* colors;           /* [n_colors][3] BGR   (gather) */
    uint8_t* atlas;                /* [S][S][3] RGB: out (gather), in (sample) */
    const int64_t* hit_face;       /* [R]   (sample) */
    const double* hit_points;      /* [R][3]   (sample) */
    float* rgb;                    /* [R][3] out   (sample) */
    int64_t V, F, R, n_colors;
    double bg_r, bg_g, bg_b;       /* the colour of a miss   (sample) */
    int32_t S, n, index_bytes, _pad;
} VdnTexArgs;
int vdn_tex_points(const VdnTexArgs* args_host, void* stream);
int vdn_tex_gather(const VdnTexArgs* args_host, void* stream);
int vdn_tex_sample(const VdnTexArgs* args_host, void* stream);

/* vdn_tex_project: one Newton step of N points towards the level set of a field whose value and gradient the caller evaluated at x,
 * held inside the ball of radius max_offset around x0. One thread per point, in double on the widened fp32 inputs:
 *   den = max((gx gx + gy gy) + gz gz, 1e-12);  y = x + (-sdf g) / den;  e = y - x0;  r = sqrt((ex ex + ey ey) + ez ez);
 *   r > max_offset: y = x0 + e (max_offset / r);   out = fp32(y).
 * Where that rounding carries out past the ball (in double, from the rounded values), every component steps to the next fp32 towards
 * x0, so |out - x0| <= max_offset holds for the stored floats. A non-finite sdf, g or result leaves the point where it was:
 * out = x. out may be x itself. */
typedef struct {
    const float* x;                /* [N][3] */
    const float* x0;               /* [N][3] */
    const float* sdf;              /* [N] */
    const float* g;                /* [N][3] */
    float* out;                    /* [N][3] */
    int64_t N;
    double max_offset;
} VdnTexProjectArgs;
int vdn_tex_project(const VdnTexProjectArgs* args_host, void* stream);

/* ---- textured meshes: texel colours from the photographs (csrc/mesh_photo.hip; vdn_hip/mesh.py: photo_colors, bake_texture(photos=)) ----
 * vdn_tex_photo: one thread per texel point p visits the cameras k = 0 .. N - 1 in that order; no atomics, so every sum has one order
 * and two runs - and two cell sizes of the grid - give the same bits. All arithmetic is double on the widened fp32 inputs, every
 * product and sum rounded on its own (the file is built without contraction), sums left to right unless bracketed; only + - * / sqrt
 * min max floor are used. x = points[p] is where the colour is looked up, y = anchors[p] (NULL: x) the texel's place on its triangle,
 * f = face[p]. The unit normal n = g / sqrt((g0 g0 + g1 g1) + g2 g2), component by component: g = normals[p], one-sided; without
 * `normals` g = e1 x e2 = (e1_1 e2_2 - e1_2 e2_1, e1_2 e2_0 - e1_0 e2_2, e1_0 e2_1 - e1_1 e2_0) of face f's record (e1 = b - a,
 * e2 = c - a), two-sided. A normal whose length is zero or not finite sees no camera. Camera k, M = P_mat[k], c = centres[k],
 * contributes iff, tested in this order:
 *   1. in front: w = ((M20 x0 + M21 x1) + M22 x2) + M23 > 0; u and v are the rows 0 and 1 likewise, divided by w: the continuous pixel
 *      position, pixel centres at integer coordinates (vdn_gen_rays' convention).
 *   2. in frame: u >= 0, (W - 1) - u >= 0, v >= 0, (H - 1) - v >= 0 (NaN fails); m = min(min(u, (W - 1) - u), min(v, (H - 1) - v));
 *      border b = min(1, m / feather) where feather > 0, else 1.
 *   3. facing: r = c - x, cos = ((n0 r0 + n1 r1) + n2 r2) / sqrt((r0 r0 + r1 r1) + r2 r2), two-sided: cos = max(cos, -cos);
 *      cos > cos_min; the weight w_k = (cos cos) b must be > 0.
 *   4. unoccluded: the any-hit walk of vdn_ray_cast from o = c along d = y - c with the window 0 < t < 1 - eps, ignoring face f, finds
 *      nothing. Ignoring the own face lets a lookup point that was moved a little under its coarse triangle keep its cameras; eps
 *      keeps the neighbours across a shared edge from hiding the texel.
 * Its colour is the bilinear value of image k at (u, v): x0 = floor(u), x1 = min(x0 + 1, W - 1), tx = u - x0, likewise in v, per
 * channel col = ((1 - tx)(1 - ty) t00 + tx (1 - ty) t10) + ((1 - tx) ty t01 + tx ty t11), t10 the tap at (x1, y0). Then
 * sum_c += w_k col, sum_w += w_k, and a w_k strictly greater than the best so far (0 at the start) makes k the best view - the lower
 * index wins ties. blend = 0: colors = fp32(sum_c / sum_w), weight = fp32(sum_w); blend = 1: the best view's col and w_k. n_views
 * counts the contributing cameras; best_view is the best in both modes. A texel no camera passes gets colour 0, weight 0, n_views 0,
 * best_view -1. A face[p] outside [0, F) sets *error = 1 (the caller zeroes it first) and writes that row as unseen: nothing is
 * indexed with it. The images are [N][H][W][3] fp32 in whatever channel order the caller holds; all image and record addressing is
 * 64-bit. Status -1: a null pointer, P, N, F, H or W below 1, blend outside {0, 1}, cos_min or eps outside [0, 1), feather negative
 * or not finite, a bad grid; -10: P, N, F, n_refs or the cell count beyond 32-bit indexing. */
typedef struct {
    const float* points;           /* [P][3] */
    const float* anchors;          /* [P][3] or NULL (= points) */
    const int32_t* face;           /* [P] */
    const float* normals;          /* [P][3] or NULL (the faces' own, two-sided) */
    const double* P_mat;           /* [N][3][4] row-major */
    const double* centres;         /* [N][3] camera centres, -M^-1 p4 */
    const float* images;           /* [N][H][W][3] in [0, 1] */
    const float* records;          /* [F][12] */
    const int32_t* cell_start;     /* [nx*ny*nz + 1] */
    const int32_t* refs;           /* [n_refs] */
    float* colors;                 /* [P][3] out */
    float* weight;                 /* [P] out */
    int32_t* n_views;              /* [P] out */
    int32_t* best_view;            /* [P] out */
    int32_t* error;                /* [1] */
    int64_t P, N, F, n_refs;
    double lo_x, lo_y, lo_z, h, margin, cos_min, feather, eps;
    int32_t nx, ny, nz, H, W, blend;
} VdnTexPhotoArgs;
int vdn_tex_photo(const VdnTexPhotoArgs* args_host, void* stream);


/* ---- learnable poses in the training step: poses.py:16-47 + 168-212, dataset.py:111-118, renderer.py:335-359 ---------------
 * vdn_gen_rays_pose: vdn_gen_rays with the camera-to-world matrix made in the kernel from camera i's LearnPose parameters,
 * c2w = make_c2w(r, t) @ init_c2w (lie_group_helper.py Exp in the reference's own fp32 expression: n = |r| + 1e-15,
 * R = I + sin(n)/n K + (1 - cos n)/n^2 K^2, K = [r]x). Same output row, near / far and pixel / mask / feature gathers. */
typedef struct {
    const float* pixels_x;     /* [B] */
    const float* pixels_y;     /* [B] */
    const float* intrinsic_inv;/* [3,3] row-major */
    const float* r;            /* [3] axis-angle of the camera (LearnPose.r[i]) */
    const float* t;            /* [3] translation (LearnPose.t[i]) */
    const float* init_c2w;     /* [4,4] row-major or NULL (identity) */
    const float* image;        /* [H,W,3] or NULL */
    const float* mask;         /* [H,W,mask_ch] or NULL (then mask = 1) */
    const float* feats;        /* [H,W,C] or NULL */
    float* out;                /* [B, out_ld] */
    float* near;               /* [B] or NULL */
    float* far;                /* [B] or NULL */
    int32_t B, H, W, C, mask_ch, out_ld;
} VdnGenRaysPoseArgs;
int vdn_gen_rays_pose(const VdnGenRaysPoseArgs* args_host, void* stream);

/* vdn_pose_adjoint: d loss / d (r, t) of camera `cam` from the ray adjoints (vdn_ray_adjoint's d_rays_o, d_rays_d, d_z, d_z_out)
 * of rays made by vdn_gen_rays_pose with the same pixels and parameters. The chain, in reverse:
 *   depths -> near / far (NeuSRenderer._attach_rays): z_out = far * c + 1/n_samples, c = (z_out - 1/n_samples) / far (0 where
 *     far == 0); the inside depths only with n_importance == 0: z = near + (far - near) * lin_samples;
 *   near / far -> rays (near_far_from_sphere): mid = -(o.d)/(d.d), near = mid - 1, far = mid + 1;
 *   rays -> c2w: rays_d = c2w[:3,:3] normalize(K^-1 p), rays_o = c2w[:3,3];
 *   c2w -> (r, t): adjoints of `@ init_c2w` and of Exp (at r = 0 exactly: dR/dr_k = [e_k]x, as torch's autograd gives).
 * Two launches on the stream: a wave per ray writes the ray's fp64 terms of d c2w to `scratch`, then ONE workgroup sums them
 * in a fixed order (no atomics: bit-reproducible) and applies the pose adjoint. Writes dense [n_cams,3] gradients, zero outside
 * row `cam`. */
typedef struct {
    const float* pixels_x;     /* [B] */
    const float* pixels_y;     /* [B] */
    const float* intrinsic_inv;/* [3,3] */
    const float* r;            /* [3] camera cam's parameters */
    const float* t;            /* [3] */
    const float* init_c2w;     /* [4,4] or NULL */
    const float* d_rays_o;     /* [B,3] */
    const float* d_rays_d;     /* [B,3] */
    const float* d_z;          /* [B,N] or NULL (read only when n_importance == 0) */
    const float* lin_samples;  /* [N] torch.linspace(0, 1, n_samples) (n_importance == 0) */
    const float* d_z_out;      /* [B,O] or NULL */
    const float* z_out;        /* [B,O] outside depths of the step (with d_z_out) */
    float* grad_r;             /* [n_cams,3] out */
    float* grad_t;             /* [n_cams,3] out */
    double* scratch;           /* [B,12] workspace */
    int32_t B, N, O, n_samples, n_importance, cam, n_cams, _pad;
} VdnPoseAdjointArgs;
int vdn_pose_adjoint(const VdnPoseAdjointArgs* args_host, void* stream);

/* ---- image evaluation: L1, PSNR and SSIM of a rendered image against its ground truth ------------------------
 * vdn_image_stats: the sums behind the image row of a results table, from `pred` and `gt` ([H][W][3] fp32, nominally in [0, 1])
 * and an optional `mask` ([H][W][mask_ch] fp32, mask_ch 1 or 3, first channel used; a pixel is in the mask when mask > 0.1, NULL:
 * every pixel is). All arithmetic is double on the widened fp32 inputs, without contraction; e = pred - gt.
 *   result[0] = number of pixels in the mask          result[1] = sum |e| m       result[2] = sum e^2 m   (m = 1 in the mask, else 0)
 *   result[3] = sum |e|                               result[4] = sum e^2         (all pixels; sums over the three channels)
 *   result[5] = sum S over the valid window centres and the three channels        result[6] = number of valid centres
 *   result[7] = the same sum over the valid centres whose centre pixel is in the mask    result[8] = their number
 *   result[9] = H W
 * S is the structural similarity of Wang et al. 2004 per channel: an 11-tap Gaussian window, sigma 1.5, taps exp(-k^2 / 4.5)
 * normalised to sum 1, applied separably (along x, then along y, each an in-order sum k = -5..5) to x, y, x x, y y, x y;
 *   vx = E[xx] - mx mx, vy = E[yy] - my my, vxy = E[xy] - mx my, C1 = 0.01^2, C2 = 0.03^2,
 *   S = ((2 (mx my) + C1) (2 vxy + C2)) / (((mx mx + my my) + C1) ((vx + vy) + C2)),
 * only where the whole window lies inside the image: centres (y + 5, x + 5), y < H - 10, x < W - 10. Identical images give S = 1
 * exactly. ssim_map (or NULL) receives fp32(((S_0 + S_1) + S_2) / 3) per valid centre, [H - 10][W - 10].
 * Two launches: one workgroup per tile of valid centres sums its share in a fixed order into partials[tile][9] (no atomics),
 * one wave then adds the tiles in a fixed order: the result is bit-reproducible. `partials` holds partials_rows >=
 * vdn_image_stats_tiles(H, W) rows of 9 doubles; it need not be initialised. Status -1: a null image or result, H < 11, W < 11,
 * mask_ch outside {1, 3} with a mask, or a workspace that is too small; -10: H W beyond 32-bit indexing. */
typedef struct {
    const float* pred;             /* [H][W][3] */
    const float* gt;               /* [H][W][3] */
    const float* mask;             /* [H][W][mask_ch] or NULL */
    double* partials;              /* [partials_rows][9] workspace */
    double* result;                /* [10] out */
    float* ssim_map;               /* [H - 10][W - 10] out, or NULL */
    int64_t partials_rows;
    int32_t H, W, mask_ch, _pad;
} VdnImageStatsArgs;
int vdn_image_stats(const VdnImageStatsArgs* args_host, void* stream);
/* the number of workgroup tiles of an H x W image = the rows of `partials` vdn_image_stats needs (0: H < 11 or W < 11) */
int vdn_image_stats_tiles(int32_t H, int32_t W);

/* ---- mesh alignment: one round of ICP against a scanned cloud (csrc/mesh_align.hip; vdn_hip/nn.py: icp) ----------
 * vdn_icp_round: one lane per source point p = src[order[t]] (order: any visiting order, or NULL). With the 3 x 4 similarity
 * M = [sR | t] (m00 .. m23, row-major, double)
 *   y_r = fp32(((m_r0 p_x + m_r1 p_y) + m_r2 p_z) + m_r3)     the products and sums in double, in this order, without contraction;
 * the nearest record of y on the target's grid by vdn_nn_query's own search (the same shells, stop rule, tie rule and
 * d = sqrtf(d2) <= max_dist test: csrc/k_nn.h), and where that is a hit q (the record's fp32 coordinates) the pair's terms, in
 * double from the widened fp32 values, go into the 19 sums of `result`:
 *   [VDN_ICP_N]        1                              [VDN_ICP_P + c]   p_c                 [VDN_ICP_Q + c]   q_c
 *   [VDN_ICP_PP]       (p_x p_x + p_y p_y) + p_z p_z  [VDN_ICP_QQ]      the same of q
 *   [VDN_ICP_QP + 3 r + c]   q_r p_c                  [VDN_ICP_RES]     (e_x e_x + e_y e_y) + e_z e_z, e = y - q (from the fp32 y)
 * p is the UNTRANSFORMED point: a solve on the sums gives the whole transform source -> target, not an increment on M.
 * dist / idx (each optional) receive vdn_nn_query's outputs for the query y: dist[i], idx[i] of source point i, +inf / -1 for a miss.
 * Two launches, no atomics: the 64 lanes of a wave add by a butterfly (every step adds the same two numbers in both lanes), a
 * workgroup's four waves in wave order into partials[block][19], and one workgroup then adds the blocks (thread j takes blocks
 * j, j + 256, .. in order, then the same butterfly and wave order): two calls on the same arguments give the same bits. A round
 * that matches nothing gives 19 zeros. `partials` holds partials_rows >= vdn_icp_round_blocks(N) rows; it need not be initialised.
 * Status -1: a null src / ref / cell_start / partials / result, N or R < 1, a bad grid (vdn_nn_query's checks), a non-finite M,
 * or a workspace that is too small; -10: N, R or the cell count do not fit 32-bit indexing. */
#define VDN_ICP_N 0
#define VDN_ICP_P 1
#define VDN_ICP_Q 4
#define VDN_ICP_PP 7
#define VDN_ICP_QQ 8
#define VDN_ICP_QP 9
#define VDN_ICP_RES 18
#define VDN_ICP_SUMS 19
typedef struct {
    const float* src;              /* [N][3] the source points, untransformed */
    const float* ref;              /* [R][4] the target's sorted packed records (VdnNnArgs.ref) */
    const int32_t* cell_start;     /* [nx*ny*nz + 1] */
    const int32_t* order;          /* [N] or NULL */
    float* dist;                   /* [N] out, or NULL */
    int64_t* idx;                  /* [N] out, or NULL */
    double* partials;              /* [partials_rows][19] workspace */
    double* result;                /* [19] out */
    double m00, m01, m02, m03, m10, m11, m12, m13, m20, m21, m22, m23;
    int64_t N, R, partials_rows;
    float lo_x, lo_y, lo_z, h, margin, max_dist;
    int32_t nx, ny, nz, _pad;
} VdnIcpArgs;
int vdn_icp_round(const VdnIcpArgs* args_host, void* stream);
/* the number of workgroups of a round over N source points = the rows of `partials` it needs (0: N < 1 or beyond 32-bit indexing) */
int vdn_icp_round_blocks(int64_t N);
#ifdef __cplusplus
}
#endif
#endif /* VDN_RENDER_H */
