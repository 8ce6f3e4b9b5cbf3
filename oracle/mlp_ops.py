"""One-layer models of the bf16 forward launches - the SDF network (vdn_sdf_mlp_fwd_bf16 mode 1, vdn_sdf_fwd_tail_bf16), and
further down the heads (vdn_rendernet_fwd_bf16) and the background network (vdn_nerf_mlp_fwd_bf16) -, parametrised by dtype:
float64 is the reference, float32 the rounding floor. Each plane the launch saves is modelled from the plane BEFORE it, as the
kernel itself saved it, and from the bf16 weights the blob holds (operand_weights; tests/test_gpu_mlp_planes.py decodes the
blob and holds it to them exactly): "teacher forcing". Nothing of the chain's accumulated bf16 error enters; what remains per
element is one fp32 accumulation, the transcendentals of one activation and one bf16 rounding.

Written from DESIGN.md section 4 (a_l, h_l), section 3a ("Scaled units"), include/vdn_render.h (VdnSdfArgs: the units of H /
V / PE; VdnChunkDesc: what a chunk holds) and oracle/neus_oracle.py. Scaled units, C = 100 log2 e:
    x   = C PE(scale p)                    the encoded input (saved plane PE, 39 valid columns)
    t_l = W_l g_{l-1} + C b_l              (layer 4: W_4 / sqrt 2 on [g_3 (217) | x (39)], folded into the image)
    g_l = log2(1 + 2^t_l) = C h_l          (saved plane H[l])
    out = W_8 g_7 / C + b_8                (feature plane: rows 1..256; sdf = out_0 / scale)

Units and comparator (as oracle/dw_ops.py *_units, oracle/sampler_ops.py judge): the unit of an element is what ONE float32
rounding of each operation that forms it may move it by,
    2^-24 (sum_k |w_k x_k| + |b|) |f'|  +  2^-23 |y| per transcendental (v_exp_f32, v_log_f32 are 1-ulp instructions)
(hidden_units, last_units, posenc_units below spell out the terms). The allowed deviation is e = max(1, 3 floor) units + the
plane's documented extra terms, floor = the float32 model's own error against the float64 model in the same units, measured on
the CPU at run time, never from the kernel; three times for the reason tests/test_gpu_ray_ops.py gives. A bf16 plane passes iff
every element lies in [bf16_down(y64 - e), bf16_up(y64 + e)]: it is a bf16 rounding, in either direction, of some value within e
of the reference. An f32 output passes iff |got - y64| <= e.

Where an operand is not bit for bit a plane the test can read - the plane contract:

| Place                    | What differs                                                    | Extra term                          | Stated in |
|--------------------------|-----------------------------------------------------------------|-------------------------------------|-----------|
| PE plane (sin, cos)      | hardware sine / cosine on a float32 argument in revolutions     | C (2^-18 + 2^-23 |arg|)             | include/vdn_render.h, VdnSdfArgs.PE |
| residue slots, layers 0  | the first 25 encoded inputs enter as bf16(x) + bf16(x - bf16(x)) | model: PE plane + bf16(x64 - PE);   | DESIGN.md 3a "bf16 accuracy"; vdn_hip/images.py sdf_streams(scaled=True) |
| and 4                    | of the kernel's own float32 x, which no plane holds             | sum_{i<25} |w_i| (e_PE,i + 2^-7 |r_i|) (a residue moved by e_PE,i may round to the neighbouring bf16) | |
| sdf                      | an f32 dot of the UNROUNDED layer-7 activations with row 0 of W_8 in f32 | 2^-9 sum |w| |g_7| / (C scale) against the model fed the saved H[7]: the planes are stored round-to-nearest-even (half a bf16 ulp; a truncating store would need 2^-8 and is not what the header states) | DESIGN.md 3a "bf16 accuracy"; include/vdn_render.h, VdnSdfArgs.H |
| sweep operand v_l        | the bf16 operand 255 v_l is a second, separate rounding of the f32 value that the saved V[l] = C v_l rounds | 2^-8 sum |w| |v| on u_l | DESIGN.md 3a "Scaled units" (sweep weights / 255); include/vdn_render.h VdnSdfArgs.V |
| softplus' in the sweep   | an 8-bit code of sigma ("keeps softplus' on the chip (8-bit)")  | one code step, |u| / 255; none where sigma is exactly 0 or 1 | include/vdn_render.h VdnSdfArgs.S; DESIGN.md 3a |
| softplus' in the sweep   | formed from the activation itself, the model's from the saved (rounded) H[l] | |u| ln 2 2^-H 2^-9 H | include/vdn_render.h VdnSdfArgs.H |
| normals                  | hardware sine / cosine in J_PE                                  | scale sum_k 2^k (2^-18 + 2^-23 |arg|) (|u_sin| + |u_cos|) | include/vdn_render.h, VdnSdfArgs.PE |
| f32 outputs of an MFMA layer (heads' out; background density, rgb, feat) | the accumulator is rounded once per k-step of 16 inputs: 2 kt roundings, each up to 2^-24 of the running sum, where the unit counts one | (2 kt - 1) 2^-24 sum |w x| (times |f'|) | include/vdn_render.h, VdnRenderNetArgs.out and VdnNerfArgs.density |
| h0 of the colour head inside the fused SDF launches (col_h[0]) | the 33rd small input, the normal's z, enters behind the MFMA accumulation as one f32 fmaf(tail, nz, acc) on the F32 normal (not on its bf16 copy in col_small) with the f32 weight column of the chunks' tails: one more rounding of the whole sum than the unit counts | 2^-24 (sum |w x| + |b| + |tail nz|) | include/vdn_render.h, vdn_sdf_color_train_bf16; vdn_hip/images.py rendering_streams ("c2") |
| col_small, columns 0..2  | the point is formed in the launch, o + d z in f32 (fused or not), unscaled | none; unit 2^-24 (|d z| + |p|) | include/vdn_render.h, vdn_sdf_color_train_bf16 |
| 1 - s_l in ex_l          | formed from the rounded s_l = 1 - 2^-H (ex_l = 100 vbar_l v_l (1 - s_l)): an absolute error of one rounding below 1, whatever the size of 1 - s_l | in the unit of EX[l]: 2^-24 ln 2 |vbar_l V[l]| | DESIGN.md section 4; include/vdn_render.h VdnSdfRbarArgs.s_from_h |
| ex_l in the split launch | it stays in its wave                                            | none: the launch gives UB and AB bit for bit as rbar then fbar, so EX is read from the two-launch run | include/vdn_render.h, vdn_sdf_bwd_split_bf16 |
| adjoints of the encoded inputs (d_dirs of the heads, d_pts4 / d_dirs of the background network, d_pts of fbar) | no plane holds them: the output is modelled in one piece from the last saved delta / ab blocks | what the accumulated adjoints may carry (2 kt roundings each, at three times the floor) through |J| <= 2^k, and the hardware trig | include/vdn_render.h VdnRenderNetBwdArgs.d_dirs, VdnNerfInputGradArgs, VdnSdfFbarArgs.d_pts |
| H[3], V[3]               | 217 outputs: columns 217..255 of the plane are not promised     | not read                            | include/vdn_render.h, VdnSdfArgs.H; images.py sdf_streams (nmap of lin3) |
| fp32 entry points: the normals, ub_0, d_pts, d_dirs, d_pts4 (a sine or cosine behind a sum) | the library sincosf, 1 ulp of a value <= 1, on a float32 argument that is one rounding of scale p (LIB_TRIG) | sum_k 2^k (2^-23 + 2^-24 |arg|) (|u_sin| + |u_cos|), times the factors in front of the sum | include/vdn_render.h, VdnSdfArgs (f32 entry points) |
| fp32 entry point: S[l]   | the hardware exponential may flush a result below 2^-126 to zero | 2^-126 where S < 2^-125             | include/vdn_render.h, VdnSdfArgs (f32 entry points) |
| fp32 entry points: every MFMA layer | nothing: the operands are the f32 planes themselves; the float32 floor is the k-ordered chain mfma_chain_f32 | none (the assumption on the instruction's two products is absorbed by the factor 3) | include/vdn_render.h, VdnSdfArgs (f32 entry points) |

The heads' forward (colour head, VDN head: small_inputs, dense_relu, dense_out) and the background network's (plain_encoding,
nerf_plane_models) are in network units, and every operand there IS a plane the test reads: their only extra terms are the
hardware sine of the encodings and the accumulation term of the f32 outputs.
The colour head that runs INSIDE the fused SDF launches (vdn_sdf_color_train_bf16, vdn_shade_fused_bf16, vdn_shade_points_bf16:
ray_rows, fused_small_inputs, fused_layer0, fused_head_plane_models) is the same network in another execution, with the two rows
of the table that name it.
The heads' backward (vdn_rendernet_bwd_bf16: head_delta_out, relu_chain_step) follows them.
So does the background network's backward (vdn_nerf_mlp_bwd_bf16: nerf_bwd_plane_models).
and its input adjoints (vdn_nerf_mlp_bwd_input_bf16: nerf_input_adjoint_models), and the SDF backward (vdn_sdf_bwd_rbar_bf16 /
vdn_sdf_bwd_fbar_bf16: pe_jacobian, sdf_rbar_step, sdf_fbar_step, sdf_d_pts_model - the closed forms of DESIGN.md section 4, which
tests/test_mlp_ops_model_cpu.py holds against torch autograd of the oracle, a double backward).
The fp32 launches (vdn_*_f32; tests/test_gpu_mlp_planes_f32.py, tests/test_mlp_f32_model_cpu.py) are held by the same models in their
fp32 forms - operand_weights(fmt=0), f32=True / chain=True, s_mode 0 / 1, sdf_plane_models_f32, sdf_bwd_models_f32 at the end of
this file -: network units, row-major f32 planes, stored="f32", the last three rows of the table.
"""
import math

import numpy as np
import torch

C = 100.0 * math.log2(math.e)
U24, U23 = 2.0 ** -24, 2.0 ** -23
LN2 = math.log(2.0)
F32_QUANTUM = 2.0 ** -149               # the spacing of the float32 subnormals
D0, N_RES = 39, 25                      # encoded inputs; residue slots behind them
TRIG_ABS, TRIG_ARG = 2.0 ** -18, 2.0 ** -23
HW_TRIG = (TRIG_ABS, TRIG_ARG)          # hardware sine / cosine (bf16 entry points): absolute error, and per unit of |arg|
LIB_TRIG = (U23, U24)                   # library sincosf (f32 entry points): 1 ulp of a value <= 1; the float32 argument is one rounding of scale p


# ---- bf16 as a set of float64 values ----------------------------------------------------------------------------------------

def bf16_rne(x):
    """float32 -> nearest bf16, ties to even (finite inputs), as float64."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def bf16_trunc(x):
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def _quantum(v):
    """Spacing of the bf16 values in the binade of |v| (8 significant bits; subnormals below 2^-126)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.maximum(e, -125) - 8)


def bf16_down(v):
    """Largest bf16 value <= v (float64 in, float64 out)."""
    v = np.asarray(v, np.float64)
    q = _quantum(v)
    return np.floor(v / q) * q


def bf16_up(v):
    """Smallest bf16 value >= v."""
    v = np.asarray(v, np.float64)
    q = _quantum(v)
    return np.ceil(v / q) * q


# ---- what the blob holds ----------------------------------------------------------------------------------------------------

class HostImages:
    """Effective weights and biases of one network on the host, with the stream plans of vdn_hip/images.py: what
    operand_weights needs of a vdn_hip.images.NetImages, without a device."""

    def __init__(self, weff, bias, streams):
        self.weff, self.bias, self.streams = weff, bias, streams

    @classmethod
    def of(cls, img):
        """From a refreshed NetImages: the float32 effective weights the device materialised."""
        weff = {n: img.weff_view(n).detach().cpu().numpy() for n in img.names}
        bias = {n: None if img.matrices[n][2] is None else img.matrices[n][2].detach().cpu().numpy() for n in img.names}
        return cls(weff, bias, img.streams)

    @classmethod
    def of_linear_state(cls, sd, streams, dtype=np.float32):
        """From a state dict of plain Linear layers (name.weight / name.bias)."""
        names = [k[:-7] for k in sd if k.endswith(".weight")]
        return cls({n: np.asarray(sd[n + ".weight"], dtype) for n in names}, {n: np.asarray(sd[n + ".bias"], dtype) for n in names}, streams)

    @classmethod
    def of_sdf_state(cls, sd, streams, dtype=np.float32, n_layers=9):
        """From a weight-normed state dict (lin{l}.weight_g / weight_v / bias): W_eff = v g / |v| per row, in `dtype`."""
        weff, bias = {}, {}
        for l in range(n_layers):
            g, v = (np.asarray(sd["lin%d.%s" % (l, k)], dtype) for k in ("weight_g", "weight_v"))
            weff["lin%d" % l] = (v * (g / np.sqrt((v * v).sum(1, keepdims=True, dtype=dtype)))).astype(dtype)
            bias["lin%d" % l] = np.asarray(sd["lin%d.bias" % l], dtype)
        return cls(weff, bias, streams)


def operand_weights(img, stream, layer, rounded=True, fmt=1):
    """Layer `layer` of `stream` as its chunks hold it (include/vdn_render.h VdnChunkDesc, csrc/prep.hip):
    W [n_pad, k_pad] = bf16_rne(float32(scale) * W_eff[nmap, kmap]) (0 where a map entry is -1), b [n_pad] =
    float32(bias_scale * bias[nmap]), tail = the float32 constants that ride behind the bias block (or None); float64 arrays.
    rounded=False: the same image without any rounding (img holding float64 weights): the exact network, for the chain test.
    fmt=0: the image as an fp32 chunk holds it - W = float32(float32(scale) * W_eff[nmap, kmap]), no bf16 rounding."""
    if not isinstance(img, HostImages):
        img = HostImages.of(img)
    L = img.streams[stream][layer]
    k_pad = len(L.kmap)
    ft = np.float32 if rounded else np.float64
    Ws, bs = [], []
    for chunk in L.chunks:
        pieces = chunk if isinstance(chunk, list) else [tuple(chunk) + (0, L.kt)]
        Wc, bc = np.zeros((32, k_pad), ft), np.zeros(32, ft)
        for pi, (name, use_bias, rowmap, kt0, ktc) in enumerate(pieces):
            src = img.weff[name].astype(ft)
            M = src.T if L.transposed else src              # M[image row's source, k's source]
            rm, km = np.asarray(rowmap), L.kmap[32 * kt0:32 * (kt0 + ktc)]
            vals = ft(L.scale) * M[np.clip(rm, 0, None)[:, None], np.clip(km, 0, None)[None, :]]
            Wc[:, 32 * kt0:32 * (kt0 + ktc)] = np.where((rm[:, None] >= 0) & (km[None, :] >= 0), vals, ft(0))
            if pi == 0 and use_bias and img.bias[name] is not None:
                bc = np.where(rm >= 0, ft(L.bias_scale) * img.bias[name].astype(ft)[np.clip(rm, 0, None)], ft(0))
        Ws.append(Wc)
        bs.append(bc)
    W = np.concatenate(Ws, 0)
    tail = None
    if L.tail is not None:
        first, stride = (L.tail[3], L.tail[4]) if len(L.tail) > 3 else (0, 1)
        tail = img.weff[L.tail[0]].astype(ft).reshape(-1)[first::stride][:L.tail[2]].astype(np.float64)
    return {"W": bf16_rne(W) if rounded and fmt == 1 else W.astype(np.float64), "b": np.concatenate(bs).astype(np.float64), "tail": tail,
            "kt": L.kt, "n_chunks": len(L.chunks)}


# ---- the layers -------------------------------------------------------------------------------------------------------------

def _t(a, dtype):
    return torch.as_tensor(np.asarray(a, np.float64)).to(dtype)


def posenc_scaled(pts, scale, dtype=torch.float64, unit_c=C):
    """x = C PE(scale p) [P,39] (embedder order: p, then sin, cos per octave), with `arg` (the argument of each column) and
    `deriv` (|d column / d arg|), float64 numpy, for posenc_units."""
    p = _t(pts, dtype) * torch.tensor(float(scale), dtype=dtype)
    cols, args, der = [p], [p], [torch.ones_like(p)]
    for k in range(6):
        a = p * float(2 ** k)
        cols += [torch.sin(a), torch.cos(a)]
        args += [a, a]
        der += [torch.cos(a).abs(), torch.sin(a).abs()]
    f = lambda ts: torch.cat(ts, -1).double().numpy()
    x = (torch.cat(cols, -1) * torch.tensor(unit_c, dtype=dtype)).double().numpy()      # (unit_c = 1: the f32 entry point, network units)
    return {"y": x, "arg": f(args), "deriv": f(der)}


def posenc_units(m):
    """float32 roundings of scale p (moves the value by |arg| |d/d arg|), of the constant C and of the product (|y| each), and one
    1-ulp sine or cosine; and the plane's extra term: the hardware sine / cosine (columns 3..38)."""
    y = np.abs(m["y"])
    trig = np.ones_like(y)
    trig[:, :3] = 0.0
    unit = U24 * (C * np.abs(m["arg"]) * m["deriv"] + 2.0 * y) + U23 * y * trig
    extra = C * (TRIG_ABS + TRIG_ARG * np.abs(m["arg"])) * trig
    return unit, extra


def hidden_operand(l, x_plane, pe_plane, x_enc, dtype=torch.float64):
    """Input of hidden layer l in its image's padded k order, and the residues r behind the encoded inputs (None without them).
    x_plane: the saved H[l-1] [P,256]; pe_plane: the saved PE [P,39]; x_enc: the model's own x in `dtype` (the residue is
    bf16(x - PE): of a value no plane holds)."""
    if l not in (0, 4):
        return _t(x_plane, dtype), None
    pe = _t(pe_plane, dtype)
    r = _t(bf16_rne((_t(x_enc, dtype)[:, :N_RES] - pe[:, :N_RES]).double().numpy()), dtype)
    if l == 0:
        return torch.cat([pe, r], -1), r
    h = _t(x_plane, dtype)[:, :224].clone()
    h[:, 256 - D0:] = 0.0                                # (not promised columns; their weights are zero)
    return torch.cat([h, pe, r], -1), r


def sdf_hidden(l, x_plane, pe, W, b, dtype=torch.float64, aten_threshold=False):
    """H[l] = log2(1 + 2^t), t = W X + b in scaled units, from the saved input plane. pe = (PE plane, model x) for layers 0, 4.
    -> y, and what hidden_units needs (float64 numpy)."""
    X, r = hidden_operand(l, x_plane, pe[0] if pe else None, pe[1] if pe else None, dtype)
    Wt, bt = _t(W, dtype), _t(b, dtype)
    t = X @ Wt.T + bt
    y = torch.clamp(t, min=0.0) + torch.log2(1.0 + torch.exp2(-t.abs()))
    if aten_threshold:                                   # (the reference's softplus returns a itself where 100 a > 20: see sdf_sweep)
        y = torch.where(t * LN2 > 20.0, t, y)
    mag = (X.abs().double() @ Wt.abs().double().T + bt.abs().double()).numpy()
    t64 = t.double()
    return {"y": y.double().numpy(), "t": t64.numpy(), "mag": mag, "sigma": torch.sigmoid(t64 * LN2).numpy(),
            "r": None if r is None else r.double().numpy()}


def hidden_units(m):
    """t: 2^-24 mag, times |dy/dt| = sigma. w = 1 + 2^t: the exponential (2^-23 2^t) and the sum (2^-24 w), through dy/dw =
    1 / (w ln 2): 2^-23 sigma / ln 2 + 2^-24 / ln 2. The logarithm: 2^-23 |y|."""
    return U24 * (m["mag"] * m["sigma"] + 2.0 * m["sigma"] / LN2 + 1.0 / LN2 + 2.0 * np.abs(m["y"]))


def residue_extra(W, r, e_pe, k0):
    """Extra term of layers 0 (k0 = 39) and 4 (k0 = 263): sum_{i<25} |w_i| (e_PE,i + 2^-7 (|r_i| + e_PE,i))."""
    d = e_pe[:, :N_RES] + 2.0 ** -7 * (np.abs(r) + e_pe[:, :N_RES])
    return d @ np.abs(W[:, k0:k0 + N_RES]).T


def sdf_last(H7, W8, b8, w8row, scale, dtype=torch.float64):
    """The last layer from the saved H[7]: feat [P,256] = rows 0..255 of the image (the network's rows 1..256; the image carries
    W_8 / C), sdf [P] = (w8row . g_7 / C + b8[256]) / scale with the float32 row that rides in the chunks' tails."""
    g = _t(H7, dtype)
    Wt, bt = _t(W8[:256], dtype), _t(b8[:256], dtype)
    feat = g @ Wt.T + bt
    w0 = _t(w8row, dtype)
    dot = g @ w0
    sdf = (dot * torch.tensor(1.0 / C, dtype=dtype) + _t(b8[256], dtype)) * torch.tensor(1.0 / float(scale), dtype=dtype)
    gm = g.abs().double()
    return {"feat": feat.double().numpy(), "feat_mag": (gm @ Wt.abs().double().T + bt.abs().double()).numpy(),
            "sdf": sdf.double().numpy(), "sdf_mag": (gm @ w0.abs().double()).numpy() / C + abs(float(b8[256]))}


def last_units(m, scale):
    """feat: the accumulation. sdf: the accumulation, then 1/C (constant and product), the bias sum, 1/scale (reciprocal and
    product): five more roundings of a value of size <= mag / scale; and its extra term (the unrounded activations)."""
    feat_unit = U24 * m["feat_mag"]
    sdf_unit = U24 * 6.0 * m["sdf_mag"] / float(scale)
    sdf_extra = 2.0 ** -9 * m["sdf_mag"] / float(scale)
    return feat_unit, sdf_unit, sdf_extra


# ---- the reverse sweep ------------------------------------------------------------------------------------------------------
# v_l = u_{l+1} . s_l, u_l = W_l^T v_l, u_8 = W_8[0, :] / scale, n = scale J_PE^T (u_0 + u_4[PE]); section 3a:
# the kernel carries 255 s_l as an 8-bit code and 255 v_l as its bf16 operand against images scaled by 1 / 255; the saved plane
# is V[l] = C v_l (include/vdn_render.h: VdnSdfArgs.V), s_l = 1 - 2^-H[l] (s_from_h = 2).

def sweep_stream_layer(l):
    """Index of the image of W_l^T in the 'full' stream (behind the 9 forward layers: W_7^T first)."""
    return 9 + (7 - l)


def sweep_u(l, V_l, Wt, dtype=torch.float64):
    """u_l = W_l^T v_l in the network's units, from the saved V[l] = C v_l and the image Wt = W_l^T / 255 (rows in the forward
    layer's padded input order). -> u [P, rows], mag = sum |w| |v|."""
    v = _t(V_l, dtype)[:, :Wt.shape[1]].clone()
    if l == 3:
        v[:, 256 - D0:] = 0.0                            # (not promised columns; their weights are zero)
    W = _t(Wt, dtype)
    k = torch.tensor(255.0 / C, dtype=dtype)
    u = (v @ W.T) * k
    return {"u": u.double().numpy(), "mag": (v.abs().double() @ W.abs().double().T).numpy() * (255.0 / C)}


def sdf_sweep(l, u_next, H_l, dtype=torch.float64, aten_threshold=False):
    """V[l] = C u_{l+1} . s_l with s_l = 1 - 2^-H[l] (the header's s_from_h = 2), columns of layer l's outputs.
    aten_threshold: the reference's softplus (fields.py:70, torch's threshold 20) has derivative exactly 1 where 100 a > 20, i.e.
    where H > log2(1 + e^20); the kernels' documented formula has no threshold (a difference of at most e^-20 = 2.1e-9 in s_l).
    Only the chain test against the oracle, which follows torch, sets it."""
    H = _t(H_l, dtype)[:, :u_next.shape[1]]
    sig = 1.0 - torch.exp2(-H)
    if aten_threshold:
        sig = torch.where(H > math.log2(1.0 + math.exp(20.0)), torch.ones_like(sig), sig)
    y = _t(u_next, dtype) * sig * torch.tensor(C, dtype=dtype)
    return {"y": y.double().numpy(), "sigma": sig.double().numpy(), "H": H.double().numpy()}


def sweep_units(m, u, mag):
    """y = C u s. Unit: the accumulation of u (2^-24 mag, times C s), four roundings of y (the code's conversion, the two
    products, the unit change), the exponential and the reciprocal behind s = 1 - 1 / (1 + 2^t) (2^-23 (1 - s) each, times C |u|).
    Extra terms (the table above): the operand v_{l+1} is a second bf16 rounding of the f32 value the saved plane rounds
    (2^-8 mag on u); s is an 8-bit code (|u| / 255; none where it is exactly 0 or 1: H = 0, or H >= 25 where 2^-H is below half
    an ulp of 1); and the model's s comes from the ROUNDED H[l], the kernel's from the activation itself: |ds| <= ln 2 2^-H 2^-9 H."""
    s, H, au = m["sigma"], m["H"], np.abs(u)
    unit = U24 * (C * s * mag + 4.0 * np.abs(m["y"])) + 2.0 * U23 * C * au * (1.0 - s)
    code = np.where((H == 0.0) | (H >= 25.0), 0.0, 1.0 / 255.0)
    extra = C * (s * 2.0 ** -8 * mag + au * code + au * LN2 * np.exp2(-H) * 2.0 ** -9 * H)
    return unit, extra


def pe_jacobian_T(pts, scale, U, dtype=torch.float64, n_freqs=6, trig=HW_TRIG):
    """n = scale J_PE(scale p)^T U [P,3] (fields.py:97-108 through the encoding), with mag = scale sum |terms| and the extra
    term of the hardware sine / cosine."""
    p = _t(pts, dtype) * torch.tensor(float(scale), dtype=dtype)
    Ut = _t(U, dtype)
    n, mag, terr = Ut[:, :3].clone(), Ut[:, :3].abs().double(), torch.zeros(len(p), 3, dtype=torch.float64)
    for k in range(n_freqs):
        f = float(2 ** k)
        us, uc = Ut[:, 3 + 6 * k:6 + 6 * k], Ut[:, 6 + 6 * k:9 + 6 * k]
        a = p * f
        n = n + f * (torch.cos(a) * us - torch.sin(a) * uc)
        mag = mag + f * ((torch.cos(a) * us).abs() + (torch.sin(a) * uc).abs()).double()
        terr = terr + f * (trig[0] + trig[1] * a.abs().double()) * (us.abs() + uc.abs()).double()
    sc = float(scale)
    return {"y": (n * torch.tensor(sc, dtype=dtype)).double().numpy(), "mag": mag.numpy() * sc, "extra": terr.numpy() * sc}


def sdf_sweep_models(ops_sweep, w8row, pts, scale, planes, pts_err=None):
    """{plane: dict(y64, y32, unit, extra, stored)} of V7..V0, U_pe and normals, each from the saved planes before it:
    V[l] from V[l+1] and H[l]; U_pe from V[0] and V[4]; normals from the launch's own U_pe. ops_sweep[l] = the image of W_l^T.
    pts_err: see sdf_plane_models (the normal moves by at most scale^2 sum_k 4^k (|u_sin| + |u_cos|) per unit of the point)."""
    out = {}
    pe_part = {}
    for l in range(7, -1, -1):
        m = {}
        for dt in (torch.float64, torch.float32):
            if l == 7:
                u = (_t(w8row, dt) * torch.tensor(1.0 / float(scale), dtype=dt)).double().numpy()[None, :].repeat(len(pts), 0)
                mag = np.zeros_like(u)
            else:
                su = sweep_u(l + 1, planes["V%d" % (l + 1)], ops_sweep[l + 1]["W"], dt)
                u, mag = su["u"], su["mag"]
                if l == 3:                               # u_4 = [d / d h_3 (217, padded to 224) | d / d x (39)]
                    pe_part[dt] = (u[:, 224:224 + D0], mag[:, 224:224 + D0])
                    u, mag = u[:, :256 - D0], mag[:, :256 - D0]
            m[dt] = (sdf_sweep(l, u, planes["H%d" % l], dt), u, mag)
        unit, extra = sweep_units(*m[torch.float64])
        out["V%d" % l] = dict(y64=m[torch.float64][0]["y"], y32=m[torch.float32][0]["y"], unit=unit, extra=extra, stored="bf16")
    if "U_pe" in planes:
        y = {}
        for dt in (torch.float64, torch.float32):
            s0 = sweep_u(0, planes["V0"], ops_sweep[0]["W"], dt)
            y[dt] = (s0["u"][:, :D0] + pe_part[dt][0], s0["mag"][:, :D0] + pe_part[dt][1])
        y64, mag = y[torch.float64]
        out["U_pe"] = dict(y64=y64, y32=y[torch.float32][0], unit=U24 * (mag + np.abs(y64)), extra=2.0 ** -8 * mag, stored="f32")
        n64, n32 = (pe_jacobian_T(pts, scale, planes["U_pe"], dt) for dt in (torch.float64, torch.float32))
        n_extra = n64["extra"]
        if pts_err is not None:
            au = np.abs(np.asarray(planes["U_pe"], np.float64))
            n_extra = n_extra + float(scale) ** 2 * pts_err * sum(4.0 ** k * (au[:, 3 + 6 * k:6 + 6 * k] + au[:, 6 + 6 * k:9 + 6 * k]) for k in range(6))
        out["normals"] = dict(y64=n64["y"], y32=n32["y"], unit=U24 * 3.0 * n64["mag"], extra=n_extra, stored="f32")
    return out


# ---- the heads' forward (vdn_rendernet_fwd_bf16): RenderingNetwork, fields.py:148-176, mode 'idr' -----------------------------
# Network units throughout. small = [points (3), PE4(view) (27), normals (3)] (plane save_small, 33 valid columns);
# h_0 = relu(W_0 [feat (256) | small] + b_0), h_l = relu(W_l h_{l-1} + b_l) (planes save_h[0..3]), out = sigmoid(W_4 h_3 + b_4)
# (squeeze_out) in f32; save_mask = (save_h > 0), exactly.

def _padded(a, n):
    return np.concatenate([a, np.zeros((len(a), n - a.shape[1]))], -1)


def small_inputs(pts, dirs, normals, dtype=torch.float64, hw_trig=True):
    """-> y [P,33] and its unit / extra term: the points and the normals are copied (no arithmetic: a bf16 rounding of the f32
    input itself), the encoded view direction is one sine or cosine of the exact product 2^k d (the hardware ones: the header's
    contract at VdnSdfArgs.PE)."""
    d = _t(dirs, dtype)
    cols, args = [_t(pts, dtype), d], [None, torch.zeros_like(d)]
    for k in range(4):
        a = d * float(2 ** k)
        cols += [torch.sin(a), torch.cos(a)]
        args += [a, a]
    cols.append(_t(normals, dtype))
    y = torch.cat(cols, -1).double().numpy()
    trig = np.zeros_like(y)
    trig[:, 6:30] = 1.0
    arg = np.zeros_like(y)
    arg[:, 6:30] = torch.cat(args[2:], -1).abs().double().numpy()
    return {"y": y, "unit": U23 * np.abs(y) * trig, "extra": (TRIG_ABS + TRIG_ARG * arg) * trig * float(hw_trig)}


def mfma_k_order(k_pad):
    """The k order of an fp32 MFMA layer (csrc/mlp_engine.h, F32::mma): for g ascending and j = 0..3 the two products k = 8 g + j and
    k = 8 g + 4 + j of one v_mfma_f32_32x32x2_f32."""
    g, j, h = np.arange(k_pad // 8)[:, None, None], np.arange(4)[None, :, None], np.arange(2)[None, None, :]
    return (8 * g + j + 4 * h).reshape(-1)


def mfma_chain_f32(x, W, b=None):
    """The float32 floor of an fp32 MFMA layer, as oracle/dw_ops.py fma_chain_f32 is of the GEMMs: x [P,K] and W [N,K] (float32
    values), acc = bias, then acc = float32(acc + w_k x_k) for k in mfma_k_order - one rounding per product, the two products of one
    instruction one after the other (include/vdn_render.h states this reading as the library's assumption) -> [P,N] as float64."""
    xT = np.ascontiguousarray(np.asarray(x, np.float32).astype(np.float64).T)       # [K, P]: the product of two float32 is exact in float64
    WT = np.ascontiguousarray(np.asarray(W, np.float32).astype(np.float64).T)       # [K, N]
    acc32 = np.zeros((xT.shape[1], WT.shape[1]), np.float32)
    if b is not None:
        acc32[:] = np.asarray(b, np.float32)[None, :]
    acc64, tmp = acc32.astype(np.float64), np.empty(acc32.shape, np.float64)
    for k in mfma_k_order(WT.shape[0]):
        if WT[k].any():                                  # (a zero column adds nothing to any accumulator)
            np.multiply(xT[k][:, None], WT[k][None, :], out=tmp)
            tmp += acc64
            acc32[...] = tmp                             # the one rounding of this product's accumulation
            acc64[...] = acc32
    return acc64


def _mm(X, Wt, bt, dtype, chain):
    """X W^T (+ b) in `dtype`; chain: the float32 evaluation is the k-ordered chain of an fp32 MFMA layer."""
    if chain and dtype == torch.float32:
        return _t(mfma_chain_f32(X.double().numpy(), Wt.double().numpy(), None if bt is None else bt.double().numpy()), dtype)
    return X @ Wt.T if bt is None else X @ Wt.T + bt


def dense_relu(x, W, b, dtype=torch.float64, chain=False):
    """relu(W x + b) from the saved input plane(s) x [P, k_pad] -> y, mag = sum |w x| + |b|."""
    X, Wt, bt = _t(x, dtype), _t(W, dtype), _t(b, dtype)
    t = _mm(X, Wt, bt, dtype, chain)
    return {"y": torch.relu(t).double().numpy(), "t": t.double().numpy(),
            "mag": (X.abs().double() @ Wt.abs().double().T + bt.abs().double()).numpy()}


def accum_extra(mag, kt):
    """The extra term of an f32 output of an MFMA layer of kt 32-wide k-tiles (the table above): one rounding of the running sum
    per k-step of 16 inputs, of which the unit counts one."""
    return (2 * kt - 1) * U24 * mag


def dense_out(x, W, b, squeeze, d_out, dtype=torch.float64, chain=False):
    """The output layer: sigmoid (squeeze_out, fields.py:170-171) or relu of W x + b, columns 0..d_out-1, with its unit:
    the accumulation through |f'| = s (1 - s), and the exponential and the reciprocal of the sigmoid (2^-23 |y| each)."""
    m = dense_relu(x, W, b, dtype, chain)
    # (chain: an fp32 MFMA layer, whose floor is its own chain - no extra term)
    extra = (lambda mag: 0.0 * mag) if chain else (lambda mag: accum_extra(mag, np.shape(W)[1] // 32))
    if not squeeze:
        return {"y": m["y"][:, :d_out], "unit": U24 * m["mag"][:, :d_out], "extra": extra(m["mag"][:, :d_out])}
    s = torch.sigmoid(_t(m["t"], torch.float64) if dtype == torch.float64 else _t(m["t"], dtype)).double().numpy()[:, :d_out]
    slope = m["mag"][:, :d_out] * s * (1.0 - s)
    return {"y": s, "unit": U24 * slope + 2.0 * U23 * s, "extra": extra(slope)}


def head_layer0_input(feat_plane, small, extra=None):
    """The operand of a head's first layer in its image's padded k order: [feature (256) | small (33, padded to 64)], and for the
    d_feature = 352 network the 96 appended channels behind them (k 320..415: vdn_hip/images.py rendering_streams)."""
    x = [feat_plane, _padded(small, 64)] + ([extra] if extra is not None else [])
    return np.concatenate(x, -1)


def head_plane_models(ops, pts, dirs, normals, feat_plane, planes, squeeze, d_out, extra=None, f32=False):
    """{plane: dict(y64, y32, unit, extra, stored)} of one vdn_rendernet_fwd_bf16 launch: small from the inputs, h0 from the
    feature plane it was given and the small plane it saved, h1..h3 and out from the plane before. ops: layers 0..4 of 'fwd'.
    extra [P,96] (d_feature = 352): the f32 input whose bf16 copy is the plane save_extra, read by layer 0 behind small."""
    # f32: vdn_rendernet_fwd_f32 - row-major f32 planes (copies are exact), the library sincosf, every float32 evaluation of a layer
    # the k-ordered chain of mfma_chain_f32, on the fmt-0 operand weights
    out = {}
    st = "f32" if f32 else "bf16"
    if extra is not None:
        e = np.asarray(extra, np.float64)
        out["extra"] = dict(y64=e, y32=e, unit=np.zeros_like(e), extra=0.0, stored=st)
    s64, s32 = (small_inputs(pts, dirs, normals, dt, hw_trig=not f32) for dt in (torch.float64, torch.float32))
    out["small"] = dict(y64=s64["y"], y32=s32["y"], unit=s64["unit"], extra=s64["extra"], stored=st)
    x = head_layer0_input(feat_plane, planes["small"], planes["extra"] if extra is not None else None)
    for l in range(4):
        m64, m32 = (dense_relu(x, ops[l]["W"], ops[l]["b"], dt, f32) for dt in (torch.float64, torch.float32))
        out["h%d" % l] = dict(y64=m64["y"], y32=m32["y"], unit=U24 * m64["mag"], extra=0.0, stored=st)
        x = planes["h%d" % l]
    o64, o32 = (dense_out(x, ops[4]["W"], ops[4]["b"], squeeze, d_out, dt, f32) for dt in (torch.float64, torch.float32))
    out["out"] = dict(y64=o64["y"], y32=o32["y"], unit=o64["unit"], extra=o64["extra"], stored="f32")
    return out


def simulate_head_forward(ops, pts, dirs, normals, feat_plane, squeeze, d_out, rnd=bf16_rne, extra=None, chain=False):
    """The CPU stand-in of the launch (float32 chain through its own bf16 planes), for the comparator's own test."""
    planes = {"small": rnd(small_inputs(pts, dirs, normals, torch.float32)["y"])}
    if extra is not None:
        planes["extra"] = rnd(extra)
    x = head_layer0_input(feat_plane, planes["small"], planes.get("extra"))
    for l in range(4):
        planes["h%d" % l] = rnd(dense_relu(x, ops[l]["W"], ops[l]["b"], torch.float32, chain)["y"])
        x = planes["h%d" % l]
    planes["out"] = dense_out(x, ops[4]["W"], ops[4]["b"], squeeze, d_out, torch.float32, chain)["y"]
    return planes


# ---- the colour head inside the fused SDF launches (csrc/k_sdf_fwd2.h MODE 2 / 3 / 4; the 'c2' stream) --------------------------
# The same network as above in another execution: the feature vector stays in registers (the bits of the feature plane), the point
# and the view direction are formed per row from the ray (MODE 4: from the normal), the first layer contracts [feat (256) | small
# columns 0..31] on the matrix pipe and takes the 33rd small input, the normal's z, as an f32 rank-1 fmaf with the weight column
# that rides in the chunks' tails. MODE 3 saves col_small / col_h[0..3] / col_out: the planes modelled here.

def ray_rows(rays_o, rays_d, z, row_points, dtype=torch.float64):
    """Per row: p = o + d z of the row's own ray and sample (UNSCALED: renderer.py:233; the SDF network's scale is not applied), that
    ray's d, and |d z| for the unit. row_points [rows]: dense point ids r * n_per_ray + s, n_per_ray = z.shape[1]."""
    ids = np.asarray(row_points, np.int64)
    r, s = ids // np.shape(z)[1], ids % np.shape(z)[1]
    o, d = _t(np.asarray(rays_o)[r], dtype), _t(np.asarray(rays_d)[r], dtype)
    dz = d * _t(np.asarray(z)[r, s], dtype)[:, None]
    return {"pts": (o + dz).double().numpy(), "dirs": d.double().numpy(), "dz": dz.abs().double().numpy()}


def fused_small_inputs(pts, dirs, normals_f32, dz=None, dtype=torch.float64):
    """The [rows, 33] small plane of the fused head: small_inputs (the trig unit and the hardware-trig extra term of PE4(d)) with
    the point's own unit - one f32 multiply-add o + d z, fused or not: 2^-24 (|d z| + |p|); dz None: the point is an input."""
    m = small_inputs(pts, dirs, normals_f32, dtype)
    if dz is not None:
        m["unit"][:, :3] = U24 * (np.asarray(dz, np.float64) + np.abs(m["y"][:, :3]))
    return m


def fused_layer0(feat_plane, small_plane, nz_f32, W, b, tail, dtype=torch.float64):
    """h0 = relu(W [feat (256) | small columns 0..31] + tail nz + b): the matrix part on the two bf16 planes, the rank-1 term on
    the F32 normal's z with the f32 tail column. mag includes |tail nz|."""
    x = np.concatenate([np.asarray(feat_plane, np.float64), np.asarray(small_plane, np.float64)[:, :32]], -1)
    X, Wt, bt = _t(x, dtype), _t(W, dtype), _t(b, dtype)
    rank1 = _t(nz_f32, dtype)[:, None] * _t(tail, dtype)[None, :]
    t = (X @ Wt.T + bt) + rank1
    mag = X.abs().double() @ Wt.abs().double().T + bt.abs().double() + rank1.abs().double()
    return {"y": torch.relu(t).double().numpy(), "t": t.double().numpy(), "mag": mag.numpy()}


def fused_head_plane_models(ops_c2, rays_o, rays_d, z, row_points, normals_f32, feat_plane, planes, squeeze, scale):
    """{plane: dict(y64, y32, unit, extra, stored)} of the colour head inside one vdn_sdf_color_train_bf16 launch: small from the
    rays and the launch's own f32 normals (rows in list order), h0 from the feature plane and the small plane it saved, h1..h3 and
    out from the plane before. ops_c2: layers 0..4 of 'c2'. `scale` (the SDF network's) does not enter: the point is unscaled and
    the normals the launch wrote already carry it; it is an argument so that a caller cannot forget that it must not."""
    del scale
    nrm = np.asarray(normals_f32, np.float32).astype(np.float64)
    out = {}
    rows = {dt: ray_rows(rays_o, rays_d, z, row_points, dt) for dt in (torch.float64, torch.float32)}
    s64, s32 = (fused_small_inputs(rows[dt]["pts"], rows[dt]["dirs"], nrm, rows[dt]["dz"], dt) for dt in (torch.float64, torch.float32))
    out["small"] = dict(y64=s64["y"], y32=s32["y"], unit=s64["unit"], extra=s64["extra"], stored="bf16")
    m64, m32 = (fused_layer0(feat_plane, planes["small"], nrm[:, 2], ops_c2[0]["W"], ops_c2[0]["b"], ops_c2[0]["tail"], dt)
                for dt in (torch.float64, torch.float32))
    # (the table at the top: the fmaf behind the accumulation is one more rounding of the whole sum)
    out["h0"] = dict(y64=m64["y"], y32=m32["y"], unit=U24 * m64["mag"], extra=U24 * m64["mag"], stored="bf16")
    x = planes["h0"]
    for l in (1, 2, 3):
        m64, m32 = (dense_relu(x, ops_c2[l]["W"], ops_c2[l]["b"], dt) for dt in (torch.float64, torch.float32))
        out["h%d" % l] = dict(y64=m64["y"], y32=m32["y"], unit=U24 * m64["mag"], extra=0.0, stored="bf16")
        x = planes["h%d" % l]
    o64, o32 = (dense_out(x, ops_c2[4]["W"], ops_c2[4]["b"], squeeze, 3, dt) for dt in (torch.float64, torch.float32))
    out["out"] = dict(y64=o64["y"], y32=o32["y"], unit=o64["unit"], extra=o64["extra"], stored="f32")
    return out


def simulate_fused_head_forward(ops_c2, pts, dirs, normals_f32, feat_plane, squeeze, rnd=bf16_rne, dtype=torch.float32, nz=None):
    """The CPU stand-in of the fused head on per-row points and directions (ray_rows, or MODE 4's own), chained through its own
    planes, each rounded by `rnd`. dtype = float32: the comparator's test; dtype = float64: the end-to-end reference of
    vdn_shade_points_bf16 (whose planes nobody saves). nz: what enters the rank-1 term instead of normals[:, 2] (planted errors)."""
    nrm = np.asarray(normals_f32, np.float32).astype(np.float64)
    planes = {"small": rnd(fused_small_inputs(pts, dirs, nrm, None, dtype)["y"])}
    planes["h0"] = rnd(fused_layer0(feat_plane, planes["small"], nrm[:, 2] if nz is None else nz, ops_c2[0]["W"], ops_c2[0]["b"],
                                    ops_c2[0]["tail"], dtype)["y"])
    for l in (1, 2, 3):
        planes["h%d" % l] = rnd(dense_relu(planes["h%d" % (l - 1)], ops_c2[l]["W"], ops_c2[l]["b"], dtype)["y"])
    planes["out"] = dense_out(planes["h3"], ops_c2[4]["W"], ops_c2[4]["b"], squeeze, 3, dtype)["y"]
    return planes


def view_down_the_normal(normals_f32):
    """MODE 4's view direction in float64 from the f32 normals the launch wrote: -g / max(|g|, 1e-12) (include/vdn_render.h,
    vdn_shade_points_bf16: a zero gradient gives a zero direction)."""
    g = np.asarray(normals_f32, np.float32).astype(np.float64)
    return -g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)


# ---- the background network's forward (vdn_nerf_mlp_fwd_bf16): NeRF, fields.py:324-353 ----------------------------------------
# pe = PE10(pts4) (84), vpe = PE4(view) (27); h_i = relu(W_i h_{i-1} + b_i), i = 0..7, layer 5 on [pe | h_4] (the skip behind layer
# 4); feature = W_f h_7 + b_f (a bf16 plane, no activation), density = w_a . h_7 + b_a; hv = relu(W_v [feature | vpe] + b_v);
# rgb = W_r hv + b_r, feat = W_d hv + b_d (f32, no activation). save_mask / save_mask_v = (save_h > 0) / (save_hv > 0), exactly.

def plain_encoding(x, n_freqs, dtype=torch.float64, hw_trig=True):
    """[x, sin(2^0 x), cos(2^0 x), ...] with its unit and extra term: x is copied (a bf16 rounding of the f32 input itself), each
    other column is one hardware sine or cosine of the exact product 2^k x (the header's contract at VdnSdfArgs.PE)."""
    xt = _t(x, dtype)
    d = xt.shape[1]
    cols, args = [xt], []
    for k in range(n_freqs):
        a = xt * float(2 ** k)
        cols += [torch.sin(a), torch.cos(a)]
        args += [a, a]
    y = torch.cat(cols, -1).double().numpy()
    trig, arg = np.zeros_like(y), np.zeros_like(y)
    trig[:, d:] = 1.0
    arg[:, d:] = torch.cat(args, -1).abs().double().numpy()
    return {"y": y, "unit": U23 * np.abs(y) * trig, "extra": (TRIG_ABS + TRIG_ARG * arg) * trig * float(hw_trig)}


def nerf_inputs_of(planes):
    """The operand of each layer from the saved planes, in its image's padded k order: {layer: x}."""
    x = {0: _padded(planes["pe"], 96)}
    for i in range(1, 8):
        x[i] = planes["h%d" % (i - 1)]
    x[5] = np.concatenate([_padded(planes["pe"], 96), planes["h4"]], -1)
    x[8] = planes["h7"]
    x[9] = np.concatenate([planes["feature"], _padded(planes["vpe"], 32)], -1)
    x[10] = planes["hv"]
    return x


def _linear(x, W, b, dtype, chain=False):
    X, Wt, bt = _t(x, dtype), _t(W, dtype), _t(b, dtype)
    return _mm(X, Wt, bt, dtype, chain).double().numpy(), (X.abs().double() @ Wt.abs().double().T + bt.abs().double()).numpy()


def nerf_plane_models(ops, pts4, dirs, planes, f32=False):
    """{plane: dict(y64, y32, unit, extra, stored)} of one launch, each from the saved planes before it. ops: layers 0..10 of
    'fwd' (8 = feature_linear + alpha_linear, 9 = views_linears.0, 10 = rgb_linear + dpt_linear)."""
    # f32: vdn_nerf_mlp_fwd_f32, as head_plane_models
    out = {}
    st = "f32" if f32 else "bf16"
    for name, src, nf in (("pe", pts4, 10), ("vpe", dirs, 4)):
        e64, e32 = plain_encoding(src, nf, torch.float64, not f32), plain_encoding(src, nf, torch.float32, not f32)
        out[name] = dict(y64=e64["y"], y32=e32["y"], unit=e64["unit"], extra=e64["extra"], stored=st)
    x = nerf_inputs_of(planes)
    for i, name in [(i, "h%d" % i) for i in range(8)] + [(9, "hv")]:
        m64, m32 = (dense_relu(x[i], ops[i]["W"], ops[i]["b"], dt, f32) for dt in (torch.float64, torch.float32))
        out[name] = dict(y64=m64["y"], y32=m32["y"], unit=U24 * m64["mag"], extra=0.0, stored=st)
    (y64, mag), (y32, _) = (_linear(x[8], ops[8]["W"], ops[8]["b"], dt, f32) for dt in (torch.float64, torch.float32))
    out["feature"] = dict(y64=y64[:, :256], y32=y32[:, :256], unit=U24 * mag[:, :256], extra=0.0, stored=st)
    out["density"] = dict(y64=y64[:, 256], y32=y32[:, 256], unit=U24 * mag[:, 256],
                          extra=0.0 if f32 else accum_extra(mag[:, 256], ops[8]["kt"]), stored="f32")
    (y64, mag), (y32, _) = (_linear(x[10], ops[10]["W"], ops[10]["b"], dt, f32) for dt in (torch.float64, torch.float32))
    ex = np.zeros_like(mag) if f32 else accum_extra(mag, ops[10]["kt"])
    out["rgb"] = dict(y64=y64[:, :3], y32=y32[:, :3], unit=U24 * mag[:, :3], extra=ex[:, :3], stored="f32")
    if y64.shape[1] > 32:                                # (with the dpt head: three more chunks)
        out["feat"] = dict(y64=y64[:, 32:128], y32=y32[:, 32:128], unit=U24 * mag[:, 32:128], extra=ex[:, 32:128], stored="f32")
    return out


def simulate_nerf_forward(ops, pts4, dirs, rnd=bf16_rne, dtype=torch.float32, chain=False):
    """The CPU stand-in of the launch (float32 chain through its own bf16 planes), for the comparator's own test. With
    dtype = float64 and rnd = identity it is the exact chain (the chain tests)."""
    f32 = dtype
    planes = {"pe": rnd(plain_encoding(pts4, 10, f32)["y"]), "vpe": rnd(plain_encoding(dirs, 4, f32)["y"])}
    for i in range(8):
        x = nerf_inputs_of({**{"h%d" % j: np.zeros((len(pts4), 256)) for j in range(8)}, "feature": np.zeros((len(pts4), 256)),
                            "hv": None, **planes})[i]
        planes["h%d" % i] = rnd(dense_relu(x, ops[i]["W"], ops[i]["b"], f32, chain)["y"])
    y, _ = _linear(planes["h7"], ops[8]["W"], ops[8]["b"], f32, chain)
    planes["feature"], planes["density"] = rnd(y[:, :256]), y[:, 256]
    x9 = np.concatenate([planes["feature"], _padded(planes["vpe"], 32)], -1)
    planes["hv"] = rnd(dense_relu(x9, ops[9]["W"], ops[9]["b"], f32, chain)["y"])
    y, _ = _linear(planes["hv"], ops[10]["W"], ops[10]["b"], f32, chain)
    planes["rgb"] = y[:, :3]
    if y.shape[1] > 32:
        planes["feat"] = y[:, 32:128]
    return planes


# ---- the heads' backward (vdn_rendernet_bwd_bf16): the delta chain of include/vdn_render.h, VdnRenderNetBwdArgs ----------------
# delta_out = g_out . f'(out) (sigmoid: out (1 - out); relu: [out > 0]); delta_h[3] = (W_4^T delta_out) . [h_3 > 0],
# delta_h[l] = (W_{l+1}^T delta_h[l+1]) . [h_l > 0]; W_0^T delta_h[0] in the first layer's padded input order = [d_feat (256) |
# d_pts (3), d PE4(view) (27), d_normals (3) | (d_extra (96))]. 'bwd' stream: W_4^T, W_3^T, W_2^T, W_1^T, W_0^T.

def relu_chain_step(delta_next, Wt, mask, dtype=torch.float64, chain=False):
    """(W^T delta_next) . mask from the saved delta plane -> y, mag (zero where the mask is: nothing but an exact 0 passes there)."""
    d, W = _t(delta_next, dtype), _t(Wt, dtype)
    d = d[:, :W.shape[1]] if d.shape[1] >= W.shape[1] else torch.cat([d, torch.zeros(len(d), W.shape[1] - d.shape[1], dtype=dtype)], -1)
    m = _t(np.asarray(mask, np.float64), dtype)
    return {"y": (_mm(d, W, None, dtype, chain) * m).double().numpy(), "mag": ((d.abs().double() @ W.abs().double().T) * m.double()).numpy()}


def head_delta_out(g_out, out, squeeze, dtype=torch.float64):
    """delta_out and its unit: for the sigmoid g o (1 - o) - as that product (1 - o: 2^-24, i.e. |g| o; two products) or as
    g (o - o^2) (o^2, the difference, the product): 2^-24 |g| (o + 2 o (1 - o)) covers both; for relu a copy of g or 0."""
    g, o = _t(g_out, dtype), _t(out, dtype)
    if not squeeze:
        return {"y": (g * (o > 0)).double().numpy(), "unit": np.zeros(g.shape)}
    y = g * o * (1.0 - o)
    return {"y": y.double().numpy(), "unit": U24 * (g.abs() * (o + 2.0 * o * (1.0 - o))).double().numpy()}


def head_bwd_plane_models(ops_bwd, g_out, out, h_planes, planes, squeeze, d_out, with_pts=True, d_extra_before=None, f32=False):
    """{plane: dict(y64, y32, unit, extra, stored)} of one vdn_rendernet_bwd_bf16 launch: delta_out from g_out and the forward's
    out, every delta_h from the delta plane after it and the forward's saved h (its mask), d_feat / d_normals / d_pts from the
    saved delta_h[0] (f32 outputs of an MFMA layer: the accumulation term). h_planes: the forward's save_h [4][P,256]."""
    res = {}
    st = "f32" if f32 else "bf16"                        # (f32: vdn_rendernet_bwd_f32, as head_plane_models)
    d64, d32 = (head_delta_out(g_out, out, squeeze, dt) for dt in (torch.float64, torch.float32))
    res["delta_out"] = dict(y64=d64["y"], y32=d32["y"], unit=d64["unit"], extra=0.0, stored=st)
    nxt = planes["delta_out"]
    for l in (3, 2, 1, 0):
        mask = h_planes[l] > 0
        m64, m32 = (relu_chain_step(nxt, ops_bwd[3 - l]["W"], mask, dt, f32) for dt in (torch.float64, torch.float32))
        res["delta_h%d" % l] = dict(y64=m64["y"], y32=m32["y"], unit=U24 * m64["mag"], extra=0.0, stored=st)
        nxt = planes["delta_h%d" % l]
    ones = np.ones((len(nxt), ops_bwd[4]["W"].shape[0]))
    m64, m32 = (relu_chain_step(nxt, ops_bwd[4]["W"], ones, dt, f32) for dt in (torch.float64, torch.float32))
    ex = np.zeros_like(m64["mag"]) if f32 else accum_extra(m64["mag"], ops_bwd[4]["kt"])
    res["d_feat"] = dict(y64=m64["y"][:, :256], y32=m32["y"][:, :256], unit=U24 * m64["mag"][:, :256], extra=0.0, stored=st)
    for name, lo in (("d_normals", 286),) + ((("d_pts", 256),) if with_pts else ()):
        res[name] = dict(y64=m64["y"][:, lo:lo + 3], y32=m32["y"][:, lo:lo + 3], unit=U24 * m64["mag"][:, lo:lo + 3],
                         extra=ex[:, lo:lo + 3], stored="f32")
    if d_extra_before is not None:                       # d_feature = 352: rows 320..415, ADDED into what d_extra held
        y64 = m64["y"][:, 320:416] + d_extra_before
        res["d_extra"] = dict(y64=y64, y32=m32["y"][:, 320:416] + d_extra_before, unit=U24 * (m64["mag"][:, 320:416] + np.abs(y64)),
                              extra=ex[:, 320:416], stored="f32")
    return res


def head_d_dirs_model(ops_bwd, delta_h0, dirs, f32=False):
    """d_dirs = J_PE4(view)^T (W_0^T delta_h[0])[259:286] [P,3]: the 27 adjoints of the encoded view are no plane, so this output
    is modelled from delta_h[0] in one piece. Unit: the Jacobian's sum; extra: the hardware sine / cosine and what the 27
    accumulated adjoints may carry (2 kt roundings each, at three times the floor), through |J| <= 2^k."""
    ones = np.ones((len(delta_h0), ops_bwd[4]["W"].shape[0]))
    r = {}
    for dt in (torch.float64, torch.float32):
        m = relu_chain_step(delta_h0, ops_bwd[4]["W"], ones, dt, f32)
        r[dt] = (pe_jacobian_T(dirs, 1.0, m["y"][:, 259:286], dt, n_freqs=4, trig=(U23, 0.0) if f32 else HW_TRIG), m["mag"][:, 259:286])
    j64, mag = r[torch.float64]
    w = np.concatenate([np.ones(3)] + [np.full(6, 2.0 ** k) for k in range(4)])
    # (f32: the library sincosf of the exact product 2^k d, and the adjoints' float32 floor is their own chain: nothing carried)
    carried = (3.0 * 2 * ops_bwd[4]["kt"] * U24 * mag * w).reshape(len(mag), 9, 3).sum(1) * (0.0 if f32 else 1.0)
    return dict(y64=j64["y"], y32=r[torch.float32][0]["y"], unit=U24 * 3.0 * j64["mag"], extra=j64["extra"] + carried, stored="f32")


def simulate_head_backward(ops_bwd, g_out, out, h_planes, squeeze, rnd=bf16_rne, chain=False):
    """The CPU stand-in of the launch (float32 chain through its own bf16 planes)."""
    planes = {"delta_out": rnd(head_delta_out(g_out, out, squeeze, torch.float32)["y"])}
    nxt = planes["delta_out"]
    for l in (3, 2, 1, 0):
        planes["delta_h%d" % l] = rnd(relu_chain_step(nxt, ops_bwd[3 - l]["W"], h_planes[l] > 0, torch.float32, chain)["y"])
        nxt = planes["delta_h%d" % l]
    u = relu_chain_step(nxt, ops_bwd[4]["W"], np.ones((len(nxt), ops_bwd[4]["W"].shape[0])), torch.float32, chain)["y"]
    planes["d_feat"], planes["d_pts"], planes["d_normals"] = rnd(u[:, :256]), u[:, 256:259], u[:, 286:289]
    return planes


# ---- the background network's backward (vdn_nerf_mlp_bwd_bf16): include/vdn_render.h, VdnNerfBwdArgs ----------------------------
# 'bwd' stream: W_out^T, W_views^T, W_head^T, W_7^T .. W_1^T. delta_o = [g_rgb (3, padded to 32) | g_feat (96)]; delta_v =
# (W_out^T delta_o) . [hv > 0]; delta_head = [(W_views^T delta_v)[feature rows] (256) | g_density (1)]; delta_h[7] = (W_head^T
# delta_head) . [h_7 > 0]; delta_h[l] = (W_{l+1}^T delta_h[l+1]) . [h_l > 0], layer 5's transposed image in its padded input
# order [pe (96) | h_4 (256)].

def nerf_bwd_plane_models(ob, g_density, g_rgb, g_feat, h_planes, hv_plane, planes, f32=False):
    """{plane: dict(y64, y32, unit, extra, stored)} of one launch, each from the saved delta plane after it and the forward's saved
    activations (their masks). ob: layers 0..9 of 'bwd'. g_feat None: without the dpt head (delta_o is [P,32])."""
    res = {}
    st = "f32" if f32 else "bf16"                        # (f32: vdn_nerf_mlp_bwd_f32, as head_plane_models)
    g_o = np.zeros((len(g_rgb), 128 if g_feat is not None else 32))
    g_o[:, :3] = g_rgb
    if g_feat is not None:
        g_o[:, 32:] = g_feat
    res["delta_o"] = dict(y64=g_o, y32=g_o, unit=np.zeros_like(g_o), extra=0.0, stored=st)
    both = {}
    for dt in (torch.float64, torch.float32):
        m = relu_chain_step(planes["delta_o"], ob[0]["W"], hv_plane > 0, dt, f32)
        u = relu_chain_step(planes["delta_v"], ob[1]["W"], np.ones((len(g_rgb), ob[1]["W"].shape[0])), dt, f32)
        both[dt] = (m, u)
    m64, u64 = both[torch.float64]
    res["delta_v"] = dict(y64=m64["y"], y32=both[torch.float32][0]["y"], unit=U24 * m64["mag"], extra=0.0, stored=st)
    gd = np.asarray(g_density, np.float64)[:, None]
    res["delta_head"] = dict(y64=np.concatenate([u64["y"][:, :256], gd], -1), y32=np.concatenate([both[torch.float32][1]["y"][:, :256], gd], -1),
                             unit=np.concatenate([U24 * u64["mag"][:, :256], np.zeros_like(gd)], -1), extra=0.0, stored=st)
    nxt = planes["delta_head"]
    for l, li in ((7, 2), (6, 3), (5, 4), (4, 5), (3, 6), (2, 7), (1, 8), (0, 9)):
        mask = h_planes[l] > 0
        if l == 4:                                        # W_5^T's rows: [pe (96) | h_4 (256)]
            mask = np.concatenate([np.zeros((len(mask), 96), bool), mask], -1)
        a64, a32 = (relu_chain_step(nxt, ob[li]["W"], mask, dt, f32) for dt in (torch.float64, torch.float32))
        sel = slice(96, 352) if l == 4 else slice(None)
        res["delta_h%d" % l] = dict(y64=a64["y"][:, sel], y32=a32["y"][:, sel], unit=U24 * a64["mag"][:, sel], extra=0.0, stored=st)
        nxt = planes["delta_h%d" % l]
    return res


def simulate_nerf_backward(ob, g_density, g_rgb, g_feat, h_planes, hv_plane, rnd=bf16_rne, dtype=torch.float32, chain=False):
    """The CPU stand-in of the launch (float32 chain through its own bf16 planes; float64 with rnd = identity: the exact chain)."""
    f32 = dtype
    g_o = np.zeros((len(g_rgb), 128 if g_feat is not None else 32))
    g_o[:, :3] = g_rgb
    if g_feat is not None:
        g_o[:, 32:] = g_feat
    planes = {"delta_o": rnd(g_o)}
    planes["delta_v"] = rnd(relu_chain_step(planes["delta_o"], ob[0]["W"], hv_plane > 0, f32, chain)["y"])
    u = relu_chain_step(planes["delta_v"], ob[1]["W"], np.ones((len(g_rgb), ob[1]["W"].shape[0])), f32, chain)["y"]
    planes["delta_head"] = rnd(np.concatenate([u[:, :256], np.asarray(g_density, np.float64)[:, None]], -1))
    nxt = planes["delta_head"]
    for l, li in ((7, 2), (6, 3), (5, 4), (4, 5), (3, 6), (2, 7), (1, 8), (0, 9)):
        mask = h_planes[l] > 0
        if l == 4:
            mask = np.concatenate([np.zeros((len(mask), 96), bool), mask], -1)
        y = relu_chain_step(nxt, ob[li]["W"], mask, f32, chain)["y"]
        planes["delta_h%d" % l] = rnd(y[:, 96:352] if l == 4 else y)
        nxt = planes["delta_h%d" % l]
    return planes


# ---- the SDF backward (vdn_sdf_bwd_rbar_bf16, vdn_sdf_bwd_fbar_bf16; DESIGN.md section 4, include/vdn_render.h) ------------------
# rbar (ascending l, forward images): ub_0 = scale J_PE g_n; vbar_l = W_l ub_l; ub_{l+1} = vbar_l . s_l; ex_l = 100 vbar_l . v_l .
# (1 - s_l) = ln 2 vbar_l . V[l] . 2^-H[l] with the saved V[l] = C v_l. ub_4 = [adjoint of u_4 over h_3 (217, padded to 224) |
# ub_0 (the encoded input's part: n reads u_0 + u_4[PE])]. fbar (descending l, 'fbar' images): ab_8 = [g_feat (256) | g_sdf / scale];
# ab_{l-1} = (W_l^T ab_l) . s_{l-1} + ex_{l-1}. UB, EX and AB are in the network's own units; s_l = 1 - 2^-H[l] from the saved
# plane in both the kernel and the model (s_from_h = 2): no extra term.

def pe_jacobian(pts, scale, g_n, dtype=torch.float64, trig=HW_TRIG):
    """ub_0 = scale J_PE(scale p) g_n [P,39], with mag (= |ub_0|: one product chain each) and the hardware-trig extra term."""
    p = _t(pts, dtype) * torch.tensor(float(scale), dtype=dtype)
    g = _t(g_n, dtype) * torch.tensor(float(scale), dtype=dtype)
    cols, ex = [g], [torch.zeros_like(g).double()]
    for k in range(6):
        f = float(2 ** k)
        a = p * f
        cols += [f * torch.cos(a) * g, -f * torch.sin(a) * g]
        e = f * (trig[0] + trig[1] * a.abs().double()) * g.abs().double()
        ex += [e, e]
    y = torch.cat(cols, -1).double().numpy()
    return {"y": y, "unit": U24 * 4.0 * np.abs(y), "extra": torch.cat(ex, -1).numpy()}


def rbar_operand(l, ub_l):
    """ub_l in the forward image's padded k order (the residue slots and the pad columns read zero)."""
    ub_l = np.asarray(ub_l, np.float64)
    if l == 0:
        return _padded(ub_l[:, :D0], 64)
    if l == 4:
        return np.concatenate([_padded(ub_l[:, :256 - D0], 224), _padded(ub_l[:, 224:224 + D0], 64)], -1)
    return ub_l


def one_minus_sigma(S_l, dtype, s_mode, aten_threshold=False):
    """(softplus', E = 1 - softplus', dE) of a loaded plane value, as VdnSdfRbarArgs.s_from_h reads it, and what the exponential and (s_mode 1) the
    rounded product 100 log2(e) h may move it by: s_mode 2: the plane holds H = 100 log2(e) h, E = 2^-H; 1: the plane holds h in the
    network's units, E = 2^-(100 log2(e) h) = exp(-100 h); 0: the plane holds softplus' itself (the fp32 forward's S), E = 1 - S
    as the kernel forms it (exact above 1/2)."""
    H = _t(S_l, dtype)
    if s_mode == 0:
        return H, 1.0 - H, np.zeros(H.shape)
    t = H if s_mode == 2 else H * torch.tensor(C, dtype=dtype)
    E = torch.exp2(-t)
    if aten_threshold:                                   # (the reference's softplus: see sdf_sweep)
        E = torch.where(t > math.log2(1.0 + math.exp(20.0)), torch.zeros_like(E), E)
    Ed, td = E.double().numpy(), t.double().numpy()
    return 1.0 - E, E, U23 * Ed + (2.0 * U24 * LN2 * td * Ed if s_mode == 1 else 0.0)


def sdf_rbar_step(l, ub_l, W, H_l, V_l, dtype=torch.float64, ex_factor=LN2, aten_threshold=False, s_mode=2, chain=False):
    """ub_{l+1} (its columns made by layer l) and ex_l from the saved ub_l, H[l] and V[l]. -> dicts with y / unit. The fp32 launch:
    ex_factor = 100 (V in the network's units), s_mode 0 or 1 (one_minus_sigma), chain (mfma_chain_f32)."""
    X, Wt = _t(rbar_operand(l, ub_l), dtype), _t(W, dtype)
    n = 256 - D0 if l == 3 else 256
    vbar = _mm(X, Wt, None, dtype, chain)[:, :n]
    mag = (X.abs().double() @ Wt.abs().double().T)[:, :n].numpy()
    V = _t(V_l, dtype)[:, :n]
    sig, E, dE = one_minus_sigma(np.asarray(H_l, np.float64)[:, :n], dtype, s_mode, aten_threshold)
    ub = vbar * sig
    # the documented order (ex_l = 100 vbar_l v_l (1 - s_l), s_l = 1 - 2^-H): 1 - s_l is formed from the ROUNDED
    # s_l, so it carries an absolute error of one rounding of a number just below 1 (2^-24), whatever its own size
    k = torch.tensor(ex_factor, dtype=dtype)
    # (network units, s_mode 0 / 1: the factor first, as DESIGN.md section 4 writes it - on the "hot" state vbar_l v_l alone passes
    # through the float32 subnormals, and a floor taken behind that would be the model's own loss, not a rounding)
    ex = vbar * V * (1.0 - sig) * k if s_mode == 2 else k * vbar * V * (1.0 - sig)
    s, Ed, Vd = sig.double().numpy(), E.double().numpy(), V.abs().double().numpy()
    vb = np.abs(vbar.double().numpy())
    # (dE = 2^-23 E in the scaled units of the bf16 launch: there the two dE terms are 2^-23 mag E and 2^-23 |ex|)
    return {"ub": ub.double().numpy(), "ub_unit": U24 * (mag * s + 2.0 * np.abs(ub.double().numpy())) + mag * dE,
            "ex": ex.double().numpy(), "ex_unit": U24 * ex_factor * Vd * (Ed * mag + vb) + 3.0 * U24 * np.abs(ex.double().numpy()) +
            ex_factor * vb * Vd * dE}


def sdf_fbar_step(l, ab_l, Wt, H_prev, EX_prev, dtype=torch.float64, aten_threshold=False, s_mode=2, chain=False):
    """ab_{l-1} = (W_l^T ab_l) . s_{l-1} + ex_{l-1} from the saved ab_l, H[l-1] and EX[l-1]."""
    A, W = _t(ab_l, dtype), _t(Wt, dtype)
    A = A[:, :W.shape[1]] if A.shape[1] >= W.shape[1] else torch.cat([A, torch.zeros(len(A), W.shape[1] - A.shape[1], dtype=dtype)], -1)
    A = torch.where((W.abs().sum(0) > 0)[None, :], A, torch.zeros_like(A))      # (columns no weight reads: the image's padding)
    n = 256 - D0 if l == 4 else 256
    t = _mm(A, W, None, dtype, chain)[:, :n]
    mag = (A.abs().double() @ W.abs().double().T)[:, :n].numpy()
    EX = _t(EX_prev, dtype)[:, :n]
    sig, E, dE = one_minus_sigma(np.asarray(H_prev, np.float64)[:, :n], dtype, s_mode, aten_threshold)
    y = (t * sig + EX).double().numpy()
    s = sig.double().numpy()
    return {"y": y, "unit": U24 * (mag * s + 2.0 * np.abs(t.double().numpy()) * s + np.abs(y)) + mag * dE}


UB_COLS = (64, 256, 256, 256, 288, 256, 256, 256, 256)


def sdf_bwd_models(ops, ops_fbar, pts, scale, g_sdf, g_feat, g_n, H, V, ub, EX, ab):
    """{plane: dict(y64, y32, unit, extra, stored)} of rbar + fbar, each block from the saved block before it. H, V, EX: lists of
    8 planes; ub: 9 blocks, ab: 9 blocks (index = layer) as the launches left them. ops: forward images 0..7; ops_fbar[l] = the
    image of W_l^T (l = 1..8)."""
    res = {}
    j64, j32 = pe_jacobian(pts, scale, g_n, torch.float64), pe_jacobian(pts, scale, g_n, torch.float32)
    res["ub0"] = dict(y64=j64["y"], y32=j32["y"], unit=j64["unit"], extra=j64["extra"], stored="bf16")
    for l in range(8):
        m64, m32 = (sdf_rbar_step(l, ub[l], ops[l]["W"], H[l], V[l], dt) for dt in (torch.float64, torch.float32))
        res["ub%d" % (l + 1)] = dict(y64=m64["ub"], y32=m32["ub"], unit=m64["ub_unit"], extra=0.0, stored="bf16")
        res["EX%d" % l] = dict(y64=m64["ex"], y32=m32["ex"], unit=m64["ex_unit"], extra=0.0, stored="bf16")
    # the encoded input's part of ub_4 is ub_0 again: a copy of the saved block
    c = np.asarray(ub[0], np.float64)[:, :D0]
    res["ub4pe"] = dict(y64=c, y32=c, unit=np.zeros_like(c), extra=0.0, stored="bf16")
    a8 = np.concatenate([np.asarray(g_feat, np.float64), np.asarray(g_sdf, np.float64)[:, None] / float(scale)], -1)
    a8_32 = np.concatenate([np.asarray(g_feat, np.float64), (np.asarray(g_sdf, np.float32) * np.float32(1.0 / scale)).astype(np.float64)[:, None]], -1)
    u8 = np.zeros_like(a8)
    u8[:, 256] = U24 * 2.0 * np.abs(a8[:, 256])
    res["ab8"] = dict(y64=a8, y32=a8_32, unit=u8, extra=0.0, stored="bf16")
    for l in range(8, 0, -1):
        m64, m32 = (sdf_fbar_step(l, ab[l], ops_fbar[l]["W"], H[l - 1], EX[l - 1], dt) for dt in (torch.float64, torch.float32))
        res["ab%d" % (l - 1)] = dict(y64=m64["y"], y32=m32["y"], unit=m64["unit"], extra=0.0, stored="bf16")
    return res


def sdf_fbar_ops(img, rounded=True):
    """The images of W_l^T of the 'fbar' stream, indexed by l (1..8; index 0 = W_0^T, read only with d_pts)."""
    return [operand_weights(img, "fbar", 8 - l, rounded) for l in range(9)]


def simulate_sdf_backward(ops, ops_fbar, pts, scale, g_sdf, g_feat, g_n, H, V, rnd=bf16_rne, dtype=torch.float32, **kw):
    """The CPU stand-in of rbar + fbar (float32 chain through its own bf16 blocks; float64 with rnd = identity: the exact chain).
    -> ub (9 blocks), EX (8 planes), ab (9 blocks, by layer). kw: ex_factor / aten_threshold of sdf_rbar_step."""
    fk = {k: v for k, v in kw.items() if k in ("aten_threshold", "s_mode", "chain")}
    ub = [rnd(_padded(pe_jacobian(pts, scale, g_n, dtype)["y"], 64))]
    EX = []
    for l in range(8):
        m = sdf_rbar_step(l, ub[l], ops[l]["W"], H[l], V[l], dtype, **kw)
        nxt = _padded(m["ub"], 256)
        if l == 3:
            nxt = np.concatenate([_padded(m["ub"], 224), ub[0]], -1)
        ub.append(rnd(nxt))
        EX.append(rnd(_padded(m["ex"], 256)))
    ab = [None] * 9
    a8 = np.concatenate([np.asarray(g_feat, np.float64), np.asarray(g_sdf, np.float64)[:, None] / float(scale)], -1)
    ab[8] = rnd(_padded(a8, 288))
    for l in range(8, 0, -1):
        ab[l - 1] = rnd(_padded(sdf_fbar_step(l, ab[l], ops_fbar[l]["W"], H[l - 1], EX[l - 1], dtype, **fk)["y"], 256))
    return ub, EX, ab


def encoding_jacobian_T(x, U, n_freqs, dtype=torch.float64, trig=HW_TRIG):
    """J^T U of the plain encoding [x, sin(2^0 x), cos(2^0 x), ...] of a d-vector: -> y [P,d], mag (sum of |terms|), the
    hardware-trig extra term, and `carry` = sum_j |J_j| e_j for a given per-column error e of U (see nerf_input_adjoint_models)."""
    xt, Ut = _t(x, dtype), _t(U, dtype)
    d = xt.shape[1]
    y, mag, terr = Ut[:, :d].clone(), Ut[:, :d].abs().double(), torch.zeros(len(xt), d, dtype=torch.float64)
    for k in range(n_freqs):
        f = float(2 ** k)
        us, uc = Ut[:, d * (1 + 2 * k):d * (2 + 2 * k)], Ut[:, d * (2 + 2 * k):d * (3 + 2 * k)]
        a = xt * f
        y = y + f * (torch.cos(a) * us - torch.sin(a) * uc)
        mag = mag + f * ((torch.cos(a) * us).abs() + (torch.sin(a) * uc).abs()).double()
        terr = terr + f * (trig[0] + trig[1] * a.abs().double()) * (us.abs() + uc.abs()).double()
    return {"y": y.double().numpy(), "mag": mag.numpy(), "extra": terr.numpy()}


def _carried(err, d, n_freqs):
    """sum over the encoding's columns of |J| <= 2^k times a per-column error [P, d (1 + 2 n_freqs)] -> [P,d]."""
    w = np.concatenate([np.ones(d)] + [np.full(2 * d, 2.0 ** k) for k in range(n_freqs)])
    return (err * w).reshape(len(err), 1 + 2 * n_freqs, d).sum(1)


def nerf_input_adjoint_models(ob, pts4, dirs, planes, f32=False):
    """d_pts4 [P,4] and d_dirs [P,3] of vdn_nerf_mlp_bwd_input_bf16 (explicit inputs: the encodings' Jacobians, no map through the
    inverted sphere) from the saved delta_h0, delta_h5 and delta_v: the adjoints of the two encodings (W_0^T delta_h0 + the encoded
    input's rows of W_5^T delta_h5; the view's rows of W_views^T delta_v) are no plane, so each output is modelled in one piece.
    Extra: the hardware trig and what the accumulated adjoints may carry (2 kt roundings each, at three times the floor)."""
    res = {}
    r = {}
    for dt in (torch.float64, torch.float32):
        a0 = relu_chain_step(planes["delta_h0"], ob[10]["W"], np.ones((len(pts4), 96)), dt, f32)
        a5 = relu_chain_step(planes["delta_h5"], ob[5]["W"], np.ones((len(pts4), 352)), dt, f32)
        av = relu_chain_step(planes["delta_v"], ob[1]["W"], np.ones((len(pts4), 288)), dt, f32)
        r[dt] = (a0["y"][:, :84] + a5["y"][:, :84], a0["mag"][:, :84] + a5["mag"][:, :84], av["y"][:, 256:283], av["mag"][:, 256:283])
    for name, x, nf, iy, d, kt in (("d_pts4", pts4, 10, 0, 4, ob[10]["kt"] + ob[5]["kt"]), ("d_dirs", dirs, 4, 2, 3, ob[1]["kt"])):
        tr = (U23, 0.0) if f32 else HW_TRIG              # (f32: the library sincosf of the exact product 2^k x; nothing carried)
        j64 = encoding_jacobian_T(x, r[torch.float64][iy], nf, torch.float64, tr)
        j32 = encoding_jacobian_T(x, r[torch.float32][iy], nf, torch.float32, tr)
        carry = _carried(3.0 * 2 * kt * U24 * r[torch.float64][iy + 1], d, nf) * (0.0 if f32 else 1.0)
        res[name] = dict(y64=j64["y"], y32=j32["y"], unit=U24 * 3.0 * j64["mag"], extra=j64["extra"] + carry, stored="f32")
    return res


def sdf_d_pts_model(ops_fbar, pts, scale, g_n, U_pe, ab0, ab4, f32=False, before=None):
    """d_pts [P,3] of vdn_sdf_bwd_fbar_bf16: scale J_PE^T a_e + the explicit x-dependence of the Jacobian in
    n = scale J_PE(x)^T U_pe, a_e = W_0^T ab_0 + (W_4^T ab_4)[encoded input's rows] the adjoint of the encoded input (no plane: the
    output is modelled in one piece from the saved ab_0, ab_4 and the forward's U_pe):
        d_pts_d = scale (J^T a_e)_d - scale^2 g_n,d sum_k 4^k (sin(2^k s x_d) U_sin,k,d + cos(2^k s x_d) U_cos,k,d).
    f32: vdn_sdf_bwd_fbar_f32 - the library sincosf (LIB_TRIG) and the adjoints' float32 floor is their own k-ordered chain, so
    nothing is carried. before [P,3]: acc_pts = 1, the output is what d_pts held + the adjoint (one more rounding in the unit)."""
    r = {}
    tr = LIB_TRIG if f32 else HW_TRIG
    for dt in (torch.float64, torch.float32):
        a0 = relu_chain_step(ab0, ops_fbar[0]["W"], np.ones((len(pts), ops_fbar[0]["W"].shape[0])), dt, f32)
        a4 = relu_chain_step(np.asarray(ab4)[:, :256], ops_fbar[4]["W"], np.ones((len(pts), 288)), dt, f32)
        ae, mag = a0["y"][:, :D0] + a4["y"][:, 224:224 + D0], a0["mag"][:, :D0] + a4["mag"][:, 224:224 + D0]
        sc = torch.tensor(float(scale), dtype=dt)
        x = _t(pts, dt) * sc
        j = encoding_jacobian_T(x.double().numpy() if dt == torch.float64 else x.numpy(), ae, 6, dt, tr)
        U, g = _t(U_pe, dt), _t(g_n, dt)
        second, smag, strig = torch.zeros_like(x), torch.zeros(x.shape, dtype=torch.float64), torch.zeros(x.shape, dtype=torch.float64)
        for k in range(6):
            f, a = float(4 ** k), x * float(2 ** k)
            us, uc = U[:, 3 + 6 * k:6 + 6 * k], U[:, 6 + 6 * k:9 + 6 * k]
            second = second + f * (torch.sin(a) * us + torch.cos(a) * uc)
            smag = smag + f * ((torch.sin(a) * us).abs() + (torch.cos(a) * uc).abs()).double()
            strig = strig + f * (tr[0] + tr[1] * a.abs().double()) * (us.abs() + uc.abs()).double()
        y = _t(j["y"], dt) * sc - sc * sc * g * second
        if before is not None:
            y = _t(before, dt) + y
        s1, s2 = float(scale), float(scale) ** 2
        r[dt] = dict(y=y.double().numpy(), mag=s1 * j["mag"] + s2 * (g.abs().double() * smag).numpy(),
                     extra=s1 * j["extra"] + s2 * (g.abs().double() * strig).numpy() +
                     s1 * _carried(3.0 * 2 * (ops_fbar[0]["kt"] + ops_fbar[4]["kt"]) * U24 * mag, 3, 6) * (0.0 if f32 else 1.0))
    m = r[torch.float64]
    unit = U24 * 4.0 * m["mag"] + (0.0 if before is None else U24 * np.abs(m["y"]))
    return dict(y64=m["y"], y32=r[torch.float32]["y"], unit=unit, extra=m["extra"], stored="f32")


# ---- the comparator ---------------------------------------------------------------------------------------------------------

def _ratio(err, unit):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / unit)          # (a zero unit - an exact zero - admits no error at all)
    return float(q.max()) if q.size else 0.0


def judge(got, y64, y32, unit, extra=0.0, stored="bf16"):
    """-> dict(ok, bound, floor, err, used, n_bad, worst): `bound` = max(1, 3 floor) units, `err` = the kernel's error in units
    beyond its extra term and (bf16) beyond a rounding of the reference: 0 when got is a bf16 neighbour of a value within `extra`;
    `used` = the largest share of an element's whole allowance e the kernel needs (<= 1 passes)."""
    got, y64, y32 = (np.asarray(a, np.float64) for a in (got, y64, y32))
    unit = np.broadcast_to(np.asarray(unit, np.float64), y64.shape)
    extra = np.broadcast_to(np.asarray(extra, np.float64), y64.shape)
    if stored == "f32":
        # below 2^-126 a float32 is spaced 2^-149 whatever its size: a result there, or a product formed from one, carries up to half
        # that spacing per rounding, which no multiple of 2^-24 |y| covers (two roundings; an exact zero still admits nothing)
        unit = np.where(unit > 0.0, unit + F32_QUANTUM, 0.0)
    floor = _ratio(np.maximum(np.abs(y32 - y64) - extra, 0.0), unit)        # (beyond the extra term, as `err` below)
    bound = max(1.0, 3.0 * floor)
    e = bound * unit + extra
    if stored == "bf16":
        ok = (got >= bf16_down(y64 - e)) & (got <= bf16_up(y64 + e))
        # the deviation got needs: above the reference, y64 + d must pass the bf16 value below got; below, the one above
        below, above = bf16_down(np.nextafter(got, -np.inf)), bf16_up(np.nextafter(got, np.inf))
        need = np.where(got > y64, below - y64, y64 - above)
    else:
        need = np.abs(got - y64)
        ok = need <= e
    ok &= np.isfinite(got)
    need = np.where(np.isfinite(need), need, np.inf)
    err = _ratio(np.maximum(need - extra, 0.0), unit)
    used = _ratio(np.maximum(need, 0.0), e)              # the share of the whole allowance (units and extra terms) the kernel uses
    bad = np.argwhere(~ok)
    return {"ok": bool(ok.all()), "bound": bound, "floor": floor, "err": err, "used": used, "n_bad": len(bad), "n": got.size,
            "worst": None if not len(bad) else tuple(int(i) for i in bad[0])}


# ---- the launch: every plane from the planes before it ------------------------------------------------------------------------

def sdf_ops(img, rounded=True):
    """Layers 0..8 of the 'full' stream (mode 1)."""
    return [operand_weights(img, "full", l, rounded) for l in range(9)]


def sdf_sweep_ops(img, rounded=True):
    """The images of W_0^T .. W_7^T of the 'full' stream, indexed by l."""
    return [operand_weights(img, "full", sweep_stream_layer(l), rounded) for l in range(8)]


def ray_points(rays_o, rays_d, z, rows):
    """The points o + d z of the dense point ids `rows` (ray * n_per_ray + sample) in float64, and pts_err [n,3]: how far the
    launch's float32 point may lie from them - the product d z and the sum are one rounding each, or one fused rounding:
    2^-24 (|d z| + |o + d z|) <= 2^-24 (|o| + 2 |d z|) - for sdf_plane_models."""
    o, d, zz = (np.asarray(a, np.float64) for a in (rays_o, rays_d, z))
    r, s = np.asarray(rows) // zz.shape[1], np.asarray(rows) % zz.shape[1]
    dz = d[r] * zz[r, s][:, None]
    return o[r] + dz, U24 * (np.abs(o[r]) + 2.0 * np.abs(dz))


def sdf_plane_models(ops, pts, scale, planes, ops_sweep=None, pts_err=None):
    """{plane: dict(y64, y32, unit, extra, stored)} of one launch, each from the saved planes before it (`planes`: PE [P,39],
    H0..H7 [P,256] as the launch left them, float64 numpy): PE, H0..H7 (H3: 217 columns), feat, sdf.
    pts_err [P,3] (the ray form: ray_points): the launch forms its point itself, within pts_err of `pts`; column (d, octave k) of
    the encoding then moves by at most C scale 2^k |d column / d arg| pts_err_d, which joins the extra term of PE and, through
    e_pe, of the residue slots of layers 0 and 4 (and of the normals)."""
    out = {}
    pe64, pe32 = posenc_scaled(pts, scale, torch.float64), posenc_scaled(pts, scale, torch.float32)
    unit, extra = posenc_units(pe64)
    if pts_err is not None:
        freq = np.concatenate([np.ones(3)] + [np.full(6, 2.0 ** k) for k in range(6)])
        extra = extra + C * float(scale) * freq * pe64["deriv"] * np.tile(np.asarray(pts_err, np.float64), (1, 13))
    out["PE"] = dict(y64=pe64["y"], y32=pe32["y"], unit=unit, extra=extra, stored="bf16")
    e_pe = max(1.0, 3.0 * _ratio(np.abs(pe32["y"] - pe64["y"]), unit)) * unit + extra
    for l in range(8):
        x_plane = planes["H%d" % (l - 1)] if l else None
        pe = (planes["PE"], pe64["y"]) if l in (0, 4) else None
        m64 = sdf_hidden(l, x_plane, pe, ops[l]["W"], ops[l]["b"], torch.float64)
        m32 = sdf_hidden(l, x_plane, (planes["PE"], pe32["y"]) if pe else None, ops[l]["W"], ops[l]["b"], torch.float32)
        n = 256 - D0 if l == 3 else 256
        extra = residue_extra(ops[l]["W"], m64["r"], e_pe, D0 if l == 0 else 224 + D0) * m64["sigma"] if pe else np.zeros_like(m64["y"])
        out["H%d" % l] = dict(y64=m64["y"][:, :n], y32=m32["y"][:, :n], unit=hidden_units(m64)[:, :n], extra=extra[:, :n], stored="bf16")
    l64 = sdf_last(planes["H7"], ops[8]["W"], ops[8]["b"], ops[8]["tail"], scale, torch.float64)
    l32 = sdf_last(planes["H7"], ops[8]["W"], ops[8]["b"], ops[8]["tail"], scale, torch.float32)
    fu, su, se = last_units(l64, scale)
    out["feat"] = dict(y64=l64["feat"], y32=l32["feat"], unit=fu, extra=0.0, stored="bf16")
    out["sdf"] = dict(y64=l64["sdf"], y32=l32["sdf"], unit=su, extra=se, stored="f32")
    if ops_sweep is not None:
        out.update(sdf_sweep_models(ops_sweep, ops[8]["tail"], pts, scale, planes, pts_err))
    return out


def simulate_sdf_forward(ops, pts, scale, rnd=bf16_rne, ops_sweep=None, sigma_of=None):
    """A stand-in for the launch on the CPU (the comparator's own test): the float32 model chained through its own planes, each
    rounded to bf16 by `rnd`; the sdf from the unrounded layer-7 activations, as the kernel forms it; with ops_sweep the reverse
    sweep with softplus' as an 8-bit code of the unrounded activations and the two separate roundings of v_l (sigma_of: a
    replacement for s = 1 - 2^-g, for planted errors)."""
    pe = posenc_scaled(pts, scale, torch.float32)["y"]
    planes = {"PE": rnd(pe)}
    g, gs = None, []
    for l in range(8):
        gs.append(g) if l else None
        g = sdf_hidden(l, planes["H%d" % (l - 1)] if l else None, (planes["PE"], pe) if l in (0, 4) else None,
                       ops[l]["W"], ops[l]["b"], torch.float32)["y"]
        planes["H%d" % l] = np.zeros((len(pe), 256))
        planes["H%d" % l][:, :g.shape[1]] = rnd(g)
    last = sdf_last(planes["H7"], ops[8]["W"], ops[8]["b"], ops[8]["tail"], scale, torch.float32)
    planes["feat"] = rnd(last["feat"])
    planes["sdf"] = sdf_last(g, ops[8]["W"], ops[8]["b"], ops[8]["tail"], scale, torch.float32)["sdf"]
    if ops_sweep is None:
        return planes
    gs = gs + [g]                                         # the unrounded activations of layers 0..7
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float64)).float()
    u = (f32(ops[8]["tail"]) * torch.tensor(1.0 / float(scale))).expand(len(pe), -1)
    pe4 = None
    for l in range(7, -1, -1):
        gl = f32(gs[l])[:, :u.shape[1]]
        sig = (1.0 - torch.exp2(-gl)) if sigma_of is None else sigma_of(l, gl)
        v255 = u * torch.round(255.0 * sig)
        planes["V%d" % l] = np.zeros((len(pe), 256))
        planes["V%d" % l][:, :v255.shape[1]] = rnd((v255 * torch.tensor(C / 255.0)).numpy())
        operand = f32(bf16_rne(v255.numpy()))
        if l == 3:
            operand = torch.cat([operand, torch.zeros(len(pe), 224 - operand.shape[1])], -1)
        u = operand @ f32(ops_sweep[l]["W"]).T
        if l == 4:
            pe4, u = u[:, 224:224 + D0], u[:, :256 - D0]
    planes["U_pe"] = (u[:, :D0] + pe4).double().numpy()
    planes["normals"] = pe_jacobian_T(pts, scale, planes["U_pe"], torch.float32)["y"]
    return planes


def judge_planes(models, planes):
    """{plane: judge(...)} of the launch's planes against sdf_plane_models of those planes."""
    res = {}
    for k, m in models.items():
        got = np.asarray(planes[k], np.float64)
        got = got[:, :m["y64"].shape[1]] if got.ndim == 2 else got
        res[k] = judge(got, m["y64"], m["y32"], m["unit"], m["extra"], m["stored"])
    return res


# ---- the fp32 SDF launches (vdn_sdf_mlp_fwd_f32 mode 1; vdn_sdf_bwd_rbar_f32 / vdn_sdf_bwd_fbar_f32 through sdf_bwd_models_f32) -------
# Network units, row-major f32 planes, the fmt-0 operand weights of sdf_streams(scaled=False): PE [P,64] = the encoding of scale p
# (39 valid); a_l = W_l H[l-1] + b_l (layer 4 on [H[3] (217) | PE], 1 / sqrt 2 in the image); H[l] = softplus(100 a_l) / 100 and
# S[l] = sigmoid(100 a_l), both from the saved H[l-1]; feat = rows 0..255 of the last image on the saved H[7], sdf = row 256 / scale;
# V[7] = w8row / scale . S[7], V[l] = (W_{l+1}^T V[l+1]) . S[l] from the saved V[l+1] and S[l]; U_pe = u_4[PE part] + u_0;
# normals = scale J_PE^T U_pe from the saved U_pe. No factor C, no residue slots, no 8-bit softplus', no bf16 rounding: every plane is
# the f32 value itself, so a plane's only allowance is max(1, 3 floor) units, floor = the float32 model in the kernel's documented
# order (mfma_chain_f32; softplus100_pair in float32), plus the library sincosf's term where a sine enters behind a sum (LIB_TRIG).

def f32_rne(a):
    """Nearest float32 as float64: the 'rounding' of a plane of the fp32 launches' stand-ins."""
    return np.asarray(a, np.float32).astype(np.float64)


def softplus100_pair(a, dtype=torch.float64, aten_threshold=False):
    """(softplus(100 a) / 100, sigmoid(100 a)). float64: the stable closed forms (aten_threshold: the reference's softplus, which
    returns a itself and derivative 1 where 100 a > 20 - the chain tests against the oracle). float32: the evaluation
    include/vdn_render.h documents for the fp32 entry point - t = 100 log2(e) a, e = 2^-|t|, u = 1 + e, h = log2(u) ln 2 / 100 +
    max(a, 0), r = 1 / u, s = a >= 0 ? r : e r - as the floor."""
    a = _t(a, dtype)
    if dtype == torch.float64:
        z = 100.0 * a
        h, s = torch.clamp(a, min=0.0) + torch.log1p(torch.exp(-z.abs())) / 100.0, torch.sigmoid(z)
        if aten_threshold:
            h, s = torch.where(z > 20.0, a, h), torch.where(z > 20.0, torch.ones_like(s), s)
        return h, s
    t = a * torch.tensor(C, dtype=dtype)
    e = torch.exp2(-t.abs())
    u = 1.0 + e
    r = 1.0 / u
    return torch.log2(u) * torch.tensor(LN2 / 100.0, dtype=dtype) + torch.clamp(a, min=0.0), torch.where(a >= 0, r, e * r)


def sdf_hidden_operand_f32(l, x_plane, pe_plane):
    """Input of hidden layer l of the unscaled stream in its image's padded k order (pad columns and columns 217.. of H[3] read
    zero weights: vdn_hip/images.py sdf_streams, kmap of lin4)."""
    pe = None if pe_plane is None else _padded(np.asarray(pe_plane, np.float64)[:, :D0], 64)
    if l == 0:
        return pe
    if l == 4:
        return np.concatenate([_padded(np.asarray(x_plane, np.float64)[:, :256 - D0], 224), pe], -1)
    return np.asarray(x_plane, np.float64)


def sdf_hidden_f32(l, x_plane, pe_plane, W, b, dtype=torch.float64, aten_threshold=False):
    a, mag = _linear(sdf_hidden_operand_f32(l, x_plane, pe_plane), W, b, dtype, chain=True)
    h, s = softplus100_pair(a, dtype, aten_threshold)
    return {"h": h.double().numpy(), "s": s.double().numpy(), "a": a, "mag": mag}


def hidden_units_f32(m):
    """(unit of H, unit of S) from the float64 model, one float32 rounding per operation, every transcendental (v_exp_f32,
    v_log_f32, v_rcp_f32) at 2^-23 |y|. With t = 100 log2(e) |a|, e = 2^-t, L = log2(1 + e), q = e / (1 + e) = min(s, 1 - s):
    H: a (2^-24 mag, through dh/da = s), the product t (constant and product: 2 2^-24 t, through dh/dt = q ln 2 / 100), the
       exponential (2^-23 e: 2^-23 q / 100), the sum 1 + e (2^-24 (1 + e): 2^-24 / 100), the logarithm (2^-23 L ln 2 / 100), the
       constant ln 2 / 100 and the final multiply-add (2^-24 (L ln 2 / 100 + |h|)).
    S: a (through ds/da = 100 s (1 - s)), t (through ds/dt = ln 2 s (1 - s)), the exponential (2^-23 s (1 - s)), the sum and the
       reciprocal (2^-24 s, 2^-23 s) and - S's own term - the product e r where a < 0 (2^-24 s; granted on both sides)."""
    s, h, mag = m["s"], np.abs(m["h"]), m["mag"]
    t = C * np.abs(m["a"])
    e = np.exp2(-t)
    L, q, w = np.log2(1.0 + e), e / (1.0 + e), s * (1.0 - s)
    unit_h = U24 * (mag * s + h + L * LN2 / 100.0 + 1.0 / 100.0 + 2.0 * t * q * LN2 / 100.0) + U23 * (q / 100.0 + L * LN2 / 100.0)
    unit_s = U24 * (mag * 100.0 * w + 2.0 * LN2 * t * w + 2.0 * s) + U23 * (w + s)
    return unit_h, unit_s


def _sweep_operand_f32(l, V_l, k_pad):
    """V[l] as the operand of W_l^T (columns 217.. of V[3] are not outputs of layer 3; their weights are zero)."""
    v = np.array(np.asarray(V_l, np.float64)[:, :k_pad])
    if l == 3:
        v = _padded(v[:, :256 - D0], k_pad)
    return v


def sdf_plane_models_f32(ops, ops_sweep, w8row, pts, scale, planes):
    """{plane: dict(y64, y32, unit, extra, stored)} of one vdn_sdf_mlp_fwd_f32 mode-1 launch with every save, each plane from the
    saved planes before it (`planes`: PE [P,39], H0..H7, S0..S7, V0..V7 [P,256], U_pe [P,39] as the launch left them). ops: layers
    0..8 of 'full', ops_sweep[l]: the image of W_l^T, both from operand_weights(fmt=0); w8row: row 0 of W_8 (float32)."""
    out = {}
    dts = (torch.float64, torch.float32)
    pe64, pe32 = (posenc_scaled(pts, scale, dt, 1.0) for dt in dts)
    trig = np.ones_like(pe64["y"])
    trig[:, :3] = 0.0
    out["PE"] = dict(y64=pe64["y"], y32=pe32["y"], unit=U24 * np.abs(pe64["arg"]) * pe64["deriv"] + U23 * np.abs(pe64["y"]) * trig,
                     extra=0.0, stored="f32")
    for l in range(8):
        n = 256 - D0 if l == 3 else 256
        m64, m32 = (sdf_hidden_f32(l, planes["H%d" % (l - 1)] if l else None, planes["PE"], ops[l]["W"], ops[l]["b"], dt) for dt in dts)
        uh, us = hidden_units_f32(m64)
        out["H%d" % l] = dict(y64=m64["h"][:, :n], y32=m32["h"][:, :n], unit=uh[:, :n], extra=0.0, stored="f32")
        # (the hardware exponential may flush a result below the smallest normal float32 to zero: include/vdn_render.h, VdnSdfArgs.S)
        flush = np.where(m64["s"] < 2.0 ** -125, 2.0 ** -126, 0.0)
        out["S%d" % l] = dict(y64=m64["s"][:, :n], y32=m32["s"][:, :n], unit=us[:, :n], extra=flush[:, :n], stored="f32")
    sc = float(scale)
    inv = {torch.float64: 1.0 / sc, torch.float32: float(np.float32(1.0) / np.float32(sc))}
    (y64, mag), (y32, _) = (_linear(planes["H7"], ops[8]["W"], ops[8]["b"], dt, chain=True) for dt in dts)
    out["feat"] = dict(y64=y64[:, :256], y32=y32[:, :256], unit=U24 * mag[:, :256], extra=0.0, stored="f32")
    sdf64, sdf32 = y64[:, 256] * inv[torch.float64], f32_rne(y32[:, 256] * inv[torch.float32])
    out["sdf"] = dict(y64=sdf64, y32=sdf32, unit=U24 * (mag[:, 256] / sc + 2.0 * np.abs(sdf64)), extra=0.0, stored="f32")
    # the sweep
    pe_part = {}
    for l in range(7, -1, -1):
        n = 256 - D0 if l == 3 else 256
        S = np.asarray(planes["S%d" % l], np.float64)[:, :n]
        r = {}
        for dt in dts:
            if l == 7:
                u = (_t(w8row, dt) * torch.tensor(inv[dt], dtype=dt)).double().numpy()[None, :].repeat(len(S), 0)
                mag = np.abs(u)                          # (the product w8row / scale: one rounding of its own)
            else:
                Wt = ops_sweep[l + 1]["W"]
                u, mag = _linear(_sweep_operand_f32(l + 1, planes["V%d" % (l + 1)], Wt.shape[1]), Wt, np.zeros(len(Wt)), dt, chain=True)
                if l == 3:                               # u_4 = [d / d h_3 (217, padded to 224) | d / d PE (39)]
                    pe_part[dt] = (u[:, 224:224 + D0], mag[:, 224:224 + D0])
            r[dt] = ((_t(u[:, :n], dt) * _t(S, dt)).double().numpy(), mag[:, :n])
        y64, mag = r[torch.float64]
        out["V%d" % l] = dict(y64=y64, y32=r[torch.float32][0], unit=U24 * (mag * S + 2.0 * np.abs(y64)), extra=0.0, stored="f32")
    r = {}
    for dt in dts:
        Wt = ops_sweep[0]["W"]
        u0, mag0 = _linear(_sweep_operand_f32(0, planes["V0"], Wt.shape[1]), Wt, np.zeros(len(Wt)), dt, chain=True)
        r[dt] = ((_t(pe_part[dt][0], dt) + _t(u0[:, :D0], dt)).double().numpy(), pe_part[dt][1] + mag0[:, :D0])
    y64, mag = r[torch.float64]
    out["U_pe"] = dict(y64=y64, y32=r[torch.float32][0], unit=U24 * (mag + np.abs(y64)), extra=0.0, stored="f32")
    n64, n32 = (pe_jacobian_T(pts, scale, planes["U_pe"], dt, trig=LIB_TRIG) for dt in dts)
    out["normals"] = dict(y64=n64["y"], y32=n32["y"], unit=U24 * 4.0 * n64["mag"], extra=n64["extra"], stored="f32")
    return out


def simulate_sdf_forward_f32(ops, ops_sweep, w8row, pts, scale, dtype=torch.float32, rnd=f32_rne, defect=None, aten_threshold=False):
    """The CPU stand-in of the launch: the chain-ordered float32 model run through its own planes (float64 with rnd = identity: the
    exact chain, for the oracle tests). defect: a planted error - "s-negated" (S = sigmoid(-100 a)), "upe-without-u4" (the PE part of
    u_4 left out of U_pe), "hw-trig" (the error the bf16 contract allows the encoding: 2^-18 absolute)."""
    P = len(pts)
    pe = posenc_scaled(pts, scale, dtype, 1.0)["y"]
    if defect == "hw-trig":
        pe[:, 3:] += TRIG_ABS
    planes = {"PE": rnd(pe)}
    for l in range(8):
        m = sdf_hidden_f32(l, planes["H%d" % (l - 1)] if l else None, planes["PE"], ops[l]["W"], ops[l]["b"], dtype, aten_threshold)
        n = m["h"].shape[1]
        planes["H%d" % l], planes["S%d" % l] = np.zeros((P, 256)), np.zeros((P, 256))
        planes["H%d" % l][:, :n], planes["S%d" % l][:, :n] = rnd(m["h"]), rnd(1.0 - m["s"] if defect == "s-negated" else m["s"])
    inv = 1.0 / float(scale) if dtype == torch.float64 else float(np.float32(1.0) / np.float32(scale))
    y, _ = _linear(planes["H7"], ops[8]["W"], ops[8]["b"], dtype, chain=True)
    planes["feat"], planes["sdf"] = rnd(y[:, :256]), rnd(y[:, 256] * inv)
    u = (_t(w8row, dtype) * torch.tensor(inv, dtype=dtype)).double().numpy()[None, :].repeat(P, 0)
    pe4 = None
    for l in range(7, -1, -1):
        n = 256 - D0 if l == 3 else 256
        planes["V%d" % l] = np.zeros((P, 256))
        planes["V%d" % l][:, :n] = rnd((_t(u[:, :n], dtype) * _t(planes["S%d" % l][:, :n], dtype)).double().numpy())
        Wt = ops_sweep[l]["W"]
        u, _ = _linear(_sweep_operand_f32(l, planes["V%d" % l], Wt.shape[1]), Wt, np.zeros(len(Wt)), dtype, chain=True)
        if l == 4:
            pe4 = u[:, 224:224 + D0]
    planes["U_pe"] = rnd(u[:, :D0] if defect == "upe-without-u4" else (_t(pe4, dtype) + _t(u[:, :D0], dtype)).double().numpy())
    planes["normals"] = rnd(pe_jacobian_T(pts, scale, planes["U_pe"], dtype)["y"])
    return planes


def sdf_ops_f32(img, rounded=True):
    """(layers 0..8 of the unscaled 'full' stream, the images of W_0^T .. W_7^T by l, those of the 'fbar' stream by l), fmt 0."""
    return ([operand_weights(img, "full", l, rounded, fmt=0) for l in range(9)],
            [operand_weights(img, "full", sweep_stream_layer(l), rounded, fmt=0) for l in range(8)],
            [operand_weights(img, "fbar", 8 - l, rounded, fmt=0) for l in range(9)])


def sdf_bwd_models_f32(ops, ops_fbar, pts, scale, g_sdf, g_feat, g_n, S, s_mode, V, ub, EX, ab):
    """{block: dict(y64, y32, unit, extra, stored)} of vdn_sdf_bwd_rbar_f32 + vdn_sdf_bwd_fbar_f32, each block from the saved block
    before it, as sdf_bwd_models: network units (ex_l = 100 vbar_l v_l (1 - s_l)), s_mode 0 - S holds the forward's softplus' planes
    (s_from_h = 0) - or 1 - S holds the H planes and softplus' = 1 - exp(-100 h) is formed from them (s_from_h = 1)."""
    res = {}
    dts = (torch.float64, torch.float32)
    j64, j32 = (pe_jacobian(pts, scale, g_n, dt, LIB_TRIG) for dt in dts)
    res["ub0"] = dict(y64=j64["y"], y32=j32["y"], unit=j64["unit"], extra=j64["extra"], stored="f32")
    for l in range(8):
        m64, m32 = (sdf_rbar_step(l, ub[l], ops[l]["W"], S[l], V[l], dt, ex_factor=100.0, s_mode=s_mode, chain=True) for dt in dts)
        res["ub%d" % (l + 1)] = dict(y64=m64["ub"], y32=m32["ub"], unit=m64["ub_unit"], extra=0.0, stored="f32")
        res["EX%d" % l] = dict(y64=m64["ex"], y32=m32["ex"], unit=m64["ex_unit"], extra=0.0, stored="f32")
    c = np.asarray(ub[0], np.float64)[:, :D0]
    res["ub4pe"] = dict(y64=c, y32=c, unit=np.zeros_like(c), extra=0.0, stored="f32")
    gs = np.asarray(g_sdf, np.float64)[:, None]
    a8 = np.concatenate([np.asarray(g_feat, np.float64), gs / float(scale)], -1)
    u8 = np.zeros_like(a8)
    u8[:, 256] = U24 * np.abs(a8[:, 256])                # (one division)
    res["ab8"] = dict(y64=a8, y32=f32_rne(a8), unit=u8, extra=0.0, stored="f32")
    for l in range(8, 0, -1):
        m64, m32 = (sdf_fbar_step(l, ab[l], ops_fbar[l]["W"], S[l - 1], EX[l - 1], dt, s_mode=s_mode, chain=True) for dt in dts)
        res["ab%d" % (l - 1)] = dict(y64=m64["y"], y32=m32["y"], unit=m64["unit"], extra=0.0, stored="f32")
    return res
