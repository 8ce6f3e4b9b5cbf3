"""The planes of the fp32 MLP launches - the path that carries the 1e-4 parity claim -, through the C ABI (include/vdn_render.h), each
held to the float64 one-layer model of oracle/mlp_ops.py evaluated on the plane BEFORE it as the launch itself saved it and on the
f32 weights the fmt-0 blob holds - which test_blob_holds_the_operand_weights_fmt0 decodes (vdn_hip/layout.py decode_chunk_f32) and
holds to operand_weights(fmt=0) exactly, for every stream of every network. The machinery is that of tests/test_gpu_mlp_planes.py;
cases: oracle/mlp_cases.py (SDF_CASES, HEAD_CASES, NERF_CASES, SDF_UPSTREAM as they are, and the silenced-unit case of
SDF_F32_CASES); what the models, the cases and the comparator are worth is proven without a GPU by tests/test_mlp_f32_model_cpu.py.

vdn_sdf_mlp_fwd_f32 mode 1 with every save: PE, H[0..7], S[0..7], feat, sdf, V[7..0], U_pe, normals; mode 0 gives the same sdf bit
for bit. vdn_sdf_bwd_rbar_f32 then vdn_sdf_bwd_fbar_f32 on the forward's own planes with s_from_h = 0 (the S planes) and
s_from_h = 1 (S points at H, softplus' = 1 - exp(-100 h) in the kernel), acc_pts = 0 and 1: every UB block, EX[l], every AB block,
d_pts. vdn_rendernet_fwd_f32 / _bwd_f32 (colour head, VDN head, the d_feature = 352 colour head) and vdn_nerf_mlp_fwd_f32 / _bwd_f32
/ _bwd_input_f32 (with and without the dpt head, once with a work list): every plane of their argument structs and the acc_* forms.
One launch per network on the OTHER weight state must be rejected; the masks of the bf16 path must be refused (-4 / -5 for the
heads, -2 / -5 for the background network) with nothing written.

Every output is pre-filled with NaN between guard bands; afterwards every promised element is finite and judged - no element
excluded, no case skipped -, the guard bands, the rows behind the last listed row and (with a work list) the outputs of every
unlisted point are untouched. Not promised, hence not judged: the pad columns of PE, small, pe and vpe, and columns 217..255 of
H[3] / S[3] / V[3] (EX[3], ab_3 alike). Of those, nmap of lin3 maps rows 217..223 to -1: zero weights and a zero bias, so the launch
writes H = softplus(0) = ln 2 / 100, S = 1/2 and V = 0 there, exactly - which the forward test also asserts -, and columns 224..255
are never written.

Bound per (case, plane): max(1, 3 x float32 floor) units + the plane's documented extra term (the library sincosf where a sine
enters behind a sum: oracle/mlp_ops.py LIB_TRIG); the floor is the float32 model in the kernel's documented k order
(mfma_chain_f32), measured on the CPU at run time. Every (case, plane) is printed with bound, floor and kernel error (pytest -rA).

Measured on the MI355X (worst over the cases of a launch; "sdf (hot)" = the weight state with saturated units in every layer;
"sdf bwd s=0 / s=1" = rbar + fbar with s_from_h = 0 / 1 over all cases and upstream gradients, "acc" = acc_pts = 1; "head acc" =
the acc_* = 1 forms). The whole file: 85 tests in 10.7 s. Behind every MFMA layer the kernel's error IS the floor, to the last
printed digit: the launch agrees with the k-ordered chain of fused multiply-adds, the reading of v_mfma_f32_32x32x2_f32 that
include/vdn_render.h assumes. Mode 0 gives mode 1's sdf bit for bit in every case. The S planes of the "hot" state use the whole
2^-126 their contract grants below 2^-125: the hardware exponential does flush there.

sdf             PE          7 cases  bound <=   2.99  floor <=  0.996  kernel error <=  0.996 units, <= 0.40 of its allowance
sdf             H0          7 cases  bound <=  16.54  floor <=  5.513  kernel error <=  5.513 units, <= 0.33 of its allowance
sdf             S0          7 cases  bound <=   9.80  floor <=  3.267  kernel error <=  3.267 units, <= 0.33 of its allowance
sdf             H1          7 cases  bound <=  12.18  floor <=  4.061  kernel error <=  4.061 units, <= 0.33 of its allowance
sdf             S1          7 cases  bound <=   9.67  floor <=  3.224  kernel error <=  3.224 units, <= 0.33 of its allowance
sdf             H2          7 cases  bound <=  12.49  floor <=  4.163  kernel error <=  4.163 units, <= 0.33 of its allowance
sdf             S2          7 cases  bound <=   9.78  floor <=  3.260  kernel error <=  3.260 units, <= 0.33 of its allowance
sdf             H3          7 cases  bound <=  11.74  floor <=  3.914  kernel error <=  3.914 units, <= 0.33 of its allowance
sdf             S3          7 cases  bound <=   9.99  floor <=  3.329  kernel error <=  3.329 units, <= 0.33 of its allowance
sdf             H4          7 cases  bound <=  11.97  floor <=  3.991  kernel error <=  3.991 units, <= 0.33 of its allowance
sdf             S4          7 cases  bound <=   9.77  floor <=  3.257  kernel error <=  3.257 units, <= 0.33 of its allowance
sdf             H5          7 cases  bound <=  12.00  floor <=  4.001  kernel error <=  4.001 units, <= 0.33 of its allowance
sdf             S5          7 cases  bound <=  12.26  floor <=  4.088  kernel error <=  4.088 units, <= 0.33 of its allowance
sdf             H6          7 cases  bound <=  13.35  floor <=  4.452  kernel error <=  4.452 units, <= 0.33 of its allowance
sdf             S6          7 cases  bound <=   9.70  floor <=  3.233  kernel error <=  3.233 units, <= 0.33 of its allowance
sdf             H7          7 cases  bound <=  13.38  floor <=  4.460  kernel error <=  4.460 units, <= 0.33 of its allowance
sdf             S7          7 cases  bound <=   9.19  floor <=  3.062  kernel error <=  3.062 units, <= 0.33 of its allowance
sdf             feat        7 cases  bound <=  27.71  floor <=  9.236  kernel error <=  9.236 units, <= 0.33 of its allowance
sdf             sdf         7 cases  bound <=  15.45  floor <=  5.150  kernel error <=  5.150 units, <= 0.33 of its allowance
sdf             V7          7 cases  bound <=   2.12  floor <=  0.707  kernel error <=  0.707 units, <= 0.33 of its allowance
sdf             V6          7 cases  bound <=  10.85  floor <=  3.615  kernel error <=  3.615 units, <= 0.33 of its allowance
sdf             V5          7 cases  bound <=  10.27  floor <=  3.424  kernel error <=  3.424 units, <= 0.33 of its allowance
sdf             V4          7 cases  bound <=  12.49  floor <=  4.164  kernel error <=  4.164 units, <= 0.33 of its allowance
sdf             V3          7 cases  bound <=  15.09  floor <=  5.029  kernel error <=  5.029 units, <= 0.33 of its allowance
sdf             V2          7 cases  bound <=   9.88  floor <=  3.294  kernel error <=  3.294 units, <= 0.33 of its allowance
sdf             V1          7 cases  bound <=  10.49  floor <=  3.496  kernel error <=  3.496 units, <= 0.33 of its allowance
sdf             V0          7 cases  bound <=  13.74  floor <=  4.581  kernel error <=  4.581 units, <= 0.33 of its allowance
sdf             U_pe        7 cases  bound <=   8.85  floor <=  2.951  kernel error <=  2.951 units, <= 0.33 of its allowance
sdf             normals     7 cases  bound <=   1.00  floor <=  0.327  kernel error <=  0.252 units, <= 0.53 of its allowance
sdf (hot)       PE          2 cases  bound <=   3.00  floor <=  1.000  kernel error <=  1.000 units, <= 0.41 of its allowance
sdf (hot)       H0          2 cases  bound <=  16.01  floor <=  5.337  kernel error <=  5.337 units, <= 0.33 of its allowance
sdf (hot)       S0          2 cases  bound <=  10.22  floor <=  3.407  kernel error <=  3.415 units, <= 1.00 of its allowance
sdf (hot)       H1          2 cases  bound <=  11.35  floor <=  3.783  kernel error <=  3.783 units, <= 0.33 of its allowance
sdf (hot)       S1          2 cases  bound <=   7.90  floor <=  2.634  kernel error <=  2.634 units, <= 0.99 of its allowance
sdf (hot)       H2          2 cases  bound <=  10.24  floor <=  3.415  kernel error <=  3.415 units, <= 0.33 of its allowance
sdf (hot)       S2          2 cases  bound <=   7.32  floor <=  2.439  kernel error <=  2.439 units, <= 0.99 of its allowance
sdf (hot)       H3          2 cases  bound <=   8.30  floor <=  2.765  kernel error <=  2.765 units, <= 0.33 of its allowance
sdf (hot)       S3          2 cases  bound <=   8.09  floor <=  2.695  kernel error <=  2.695 units, <= 1.00 of its allowance
sdf (hot)       H4          2 cases  bound <=  11.08  floor <=  3.693  kernel error <=  3.693 units, <= 0.33 of its allowance
sdf (hot)       S4          2 cases  bound <=   8.23  floor <=  2.744  kernel error <=  2.744 units, <= 0.98 of its allowance
sdf (hot)       H5          2 cases  bound <=  10.65  floor <=  3.551  kernel error <=  3.551 units, <= 0.33 of its allowance
sdf (hot)       S5          2 cases  bound <=   7.16  floor <=  2.387  kernel error <=  2.387 units, <= 0.99 of its allowance
sdf (hot)       H6          2 cases  bound <=   9.11  floor <=  3.037  kernel error <=  3.037 units, <= 0.33 of its allowance
sdf (hot)       S6          2 cases  bound <=   8.75  floor <=  2.917  kernel error <=  2.917 units, <= 1.00 of its allowance
sdf (hot)       H7          2 cases  bound <=   9.70  floor <=  3.233  kernel error <=  3.233 units, <= 0.33 of its allowance
sdf (hot)       S7          2 cases  bound <=   7.51  floor <=  2.502  kernel error <=  2.491 units, <= 0.98 of its allowance
sdf (hot)       feat        2 cases  bound <=  36.26  floor <= 12.085  kernel error <= 12.085 units, <= 0.33 of its allowance
sdf (hot)       sdf         2 cases  bound <=   8.73  floor <=  2.910  kernel error <=  2.910 units, <= 0.33 of its allowance
sdf (hot)       V7          2 cases  bound <=   2.10  floor <=  0.700  kernel error <=  0.700 units, <= 0.33 of its allowance
sdf (hot)       V6          2 cases  bound <=   7.19  floor <=  2.395  kernel error <=  2.395 units, <= 0.33 of its allowance
sdf (hot)       V5          2 cases  bound <=   8.35  floor <=  2.784  kernel error <=  2.784 units, <= 0.33 of its allowance
sdf (hot)       V4          2 cases  bound <=   8.84  floor <=  2.947  kernel error <=  2.947 units, <= 0.33 of its allowance
sdf (hot)       V3          2 cases  bound <=   9.63  floor <=  3.211  kernel error <=  3.211 units, <= 0.33 of its allowance
sdf (hot)       V2          2 cases  bound <=   9.38  floor <=  3.126  kernel error <=  3.126 units, <= 0.33 of its allowance
sdf (hot)       V1          2 cases  bound <=   8.56  floor <=  2.853  kernel error <=  2.853 units, <= 0.33 of its allowance
sdf (hot)       V0          2 cases  bound <=   7.92  floor <=  2.638  kernel error <=  2.638 units, <= 0.33 of its allowance
sdf (hot)       U_pe        2 cases  bound <=   8.10  floor <=  2.701  kernel error <=  2.701 units, <= 0.33 of its allowance
sdf (hot)       normals     2 cases  bound <=   1.00  floor <=  0.076  kernel error <=  0.279 units, <= 0.48 of its allowance
sdf bwd s=0     ub0        13 cases  bound <=   1.00  floor <=  0.250  kernel error <=  0.250 units, <= 0.89 of its allowance
sdf bwd s=0     ub1        13 cases  bound <=  12.33  floor <=  4.111  kernel error <=  4.111 units, <= 0.33 of its allowance
sdf bwd s=0     EX0        13 cases  bound <=  11.87  floor <=  3.957  kernel error <=  3.957 units, <= 0.33 of its allowance
sdf bwd s=0     ub2        13 cases  bound <=  10.88  floor <=  3.628  kernel error <=  3.628 units, <= 0.33 of its allowance
sdf bwd s=0     EX1        13 cases  bound <=   8.21  floor <=  2.738  kernel error <=  2.738 units, <= 0.33 of its allowance
sdf bwd s=0     ub3        13 cases  bound <=  11.00  floor <=  3.668  kernel error <=  3.668 units, <= 0.33 of its allowance
sdf bwd s=0     EX2        13 cases  bound <=   8.58  floor <=  2.859  kernel error <=  2.859 units, <= 0.33 of its allowance
sdf bwd s=0     ub4        13 cases  bound <=  10.71  floor <=  3.570  kernel error <=  3.570 units, <= 0.33 of its allowance
sdf bwd s=0     EX3        13 cases  bound <=   7.90  floor <=  2.632  kernel error <=  2.632 units, <= 0.33 of its allowance
sdf bwd s=0     ub5        13 cases  bound <=  11.98  floor <=  3.994  kernel error <=  3.994 units, <= 0.33 of its allowance
sdf bwd s=0     EX4        13 cases  bound <=   9.83  floor <=  3.277  kernel error <=  3.277 units, <= 0.33 of its allowance
sdf bwd s=0     ub6        13 cases  bound <=  12.83  floor <=  4.277  kernel error <=  4.277 units, <= 0.33 of its allowance
sdf bwd s=0     EX5        13 cases  bound <=   9.92  floor <=  3.306  kernel error <=  3.306 units, <= 0.33 of its allowance
sdf bwd s=0     ub7        13 cases  bound <=  12.66  floor <=  4.222  kernel error <=  4.222 units, <= 0.33 of its allowance
sdf bwd s=0     EX6        13 cases  bound <=   7.99  floor <=  2.663  kernel error <=  2.663 units, <= 0.33 of its allowance
sdf bwd s=0     ub8        13 cases  bound <=  10.22  floor <=  3.407  kernel error <=  3.407 units, <= 0.33 of its allowance
sdf bwd s=0     EX7        13 cases  bound <=   8.26  floor <=  2.753  kernel error <=  2.753 units, <= 0.33 of its allowance
sdf bwd s=0     ub4pe      13 cases  bound <=   1.00  floor <=  0.000  kernel error <=  0.000 units, <= 0.00 of its allowance
sdf bwd s=0     ab8        13 cases  bound <=   2.00  floor <=  0.666  kernel error <=  0.666 units, <= 0.33 of its allowance
sdf bwd s=0     ab7        13 cases  bound <=   7.20  floor <=  2.400  kernel error <=  2.504 units, <= 0.36 of its allowance
sdf bwd s=0     ab6        13 cases  bound <=  11.21  floor <=  3.738  kernel error <=  3.903 units, <= 0.36 of its allowance
sdf bwd s=0     ab5        13 cases  bound <=  10.74  floor <=  3.581  kernel error <=  3.535 units, <= 0.34 of its allowance
sdf bwd s=0     ab4        13 cases  bound <=  10.65  floor <=  3.552  kernel error <=  3.552 units, <= 0.35 of its allowance
sdf bwd s=0     ab3        13 cases  bound <=  10.86  floor <=  3.620  kernel error <=  3.620 units, <= 0.35 of its allowance
sdf bwd s=0     ab2        13 cases  bound <=   9.31  floor <=  3.103  kernel error <=  3.155 units, <= 0.34 of its allowance
sdf bwd s=0     ab1        13 cases  bound <=   9.92  floor <=  3.308  kernel error <=  3.225 units, <= 0.34 of its allowance
sdf bwd s=0     ab0        13 cases  bound <=  10.19  floor <=  3.396  kernel error <=  3.396 units, <= 0.34 of its allowance
sdf bwd s=0     d_pts      13 cases  bound <=   8.01  floor <=  2.672  kernel error <=  2.928 units, <= 0.76 of its allowance
sdf bwd s=0 acc d_pts      13 cases  bound <=   6.76  floor <=  2.252  kernel error <=  2.477 units, <= 0.62 of its allowance
sdf bwd s=1     ub0        13 cases  bound <=   1.00  floor <=  0.250  kernel error <=  0.250 units, <= 0.89 of its allowance
sdf bwd s=1     ub1        13 cases  bound <=  10.49  floor <=  3.498  kernel error <=  3.498 units, <= 0.33 of its allowance
sdf bwd s=1     EX0        13 cases  bound <=  11.31  floor <=  3.770  kernel error <=  3.770 units, <= 0.35 of its allowance
sdf bwd s=1     ub2        13 cases  bound <=   9.22  floor <=  3.072  kernel error <=  3.072 units, <= 0.33 of its allowance
sdf bwd s=1     EX1        13 cases  bound <=   7.37  floor <=  2.457  kernel error <=  2.457 units, <= 0.33 of its allowance
sdf bwd s=1     ub3        13 cases  bound <=   9.37  floor <=  3.124  kernel error <=  3.124 units, <= 0.33 of its allowance
sdf bwd s=1     EX2        13 cases  bound <=   6.52  floor <=  2.172  kernel error <=  2.172 units, <= 0.33 of its allowance
sdf bwd s=1     ub4        13 cases  bound <=   9.99  floor <=  3.331  kernel error <=  3.331 units, <= 0.33 of its allowance
sdf bwd s=1     EX3        13 cases  bound <=   9.17  floor <=  3.056  kernel error <=  3.056 units, <= 0.33 of its allowance
sdf bwd s=1     ub5        13 cases  bound <=   9.58  floor <=  3.195  kernel error <=  3.195 units, <= 0.33 of its allowance
sdf bwd s=1     EX4        13 cases  bound <=   8.13  floor <=  2.709  kernel error <=  2.709 units, <= 0.34 of its allowance
sdf bwd s=1     ub6        13 cases  bound <=  10.10  floor <=  3.367  kernel error <=  3.367 units, <= 0.33 of its allowance
sdf bwd s=1     EX5        13 cases  bound <=  10.34  floor <=  3.448  kernel error <=  3.448 units, <= 0.33 of its allowance
sdf bwd s=1     ub7        13 cases  bound <=   9.75  floor <=  3.251  kernel error <=  3.251 units, <= 0.33 of its allowance
sdf bwd s=1     EX6        13 cases  bound <=   6.58  floor <=  2.195  kernel error <=  2.195 units, <= 0.33 of its allowance
sdf bwd s=1     ub8        13 cases  bound <=  11.60  floor <=  3.867  kernel error <=  3.867 units, <= 0.33 of its allowance
sdf bwd s=1     EX7        13 cases  bound <=   7.18  floor <=  2.394  kernel error <=  2.394 units, <= 0.33 of its allowance
sdf bwd s=1     ub4pe      13 cases  bound <=   1.00  floor <=  0.000  kernel error <=  0.000 units, <= 0.00 of its allowance
sdf bwd s=1     ab8        13 cases  bound <=   2.00  floor <=  0.666  kernel error <=  0.666 units, <= 0.33 of its allowance
sdf bwd s=1     ab7        13 cases  bound <=   7.12  floor <=  2.372  kernel error <=  2.152 units, <= 0.33 of its allowance
sdf bwd s=1     ab6        13 cases  bound <=  11.06  floor <=  3.688  kernel error <=  3.943 units, <= 0.37 of its allowance
sdf bwd s=1     ab5        13 cases  bound <=   9.85  floor <=  3.284  kernel error <=  3.284 units, <= 0.33 of its allowance
sdf bwd s=1     ab4        13 cases  bound <=   9.42  floor <=  3.141  kernel error <=  3.141 units, <= 0.33 of its allowance
sdf bwd s=1     ab3        13 cases  bound <=   9.33  floor <=  3.109  kernel error <=  3.109 units, <= 0.33 of its allowance
sdf bwd s=1     ab2        13 cases  bound <=   9.54  floor <=  3.181  kernel error <=  3.181 units, <= 0.33 of its allowance
sdf bwd s=1     ab1        13 cases  bound <=   9.04  floor <=  3.015  kernel error <=  3.015 units, <= 0.33 of its allowance
sdf bwd s=1     ab0        13 cases  bound <=   9.17  floor <=  3.057  kernel error <=  3.057 units, <= 0.35 of its allowance
sdf bwd s=1     d_pts      13 cases  bound <=   4.30  floor <=  1.433  kernel error <=  1.487 units, <= 0.84 of its allowance
sdf bwd s=1 acc d_pts      13 cases  bound <=   3.40  floor <=  1.133  kernel error <=  1.315 units, <= 0.82 of its allowance
head            small       5 cases  bound <=   1.61  floor <=  0.535  kernel error <=  0.957 units, <= 0.61 of its allowance
head            h0          5 cases  bound <=  11.47  floor <=  3.824  kernel error <=  3.824 units, <= 0.33 of its allowance
head            h1          5 cases  bound <=  14.34  floor <=  4.779  kernel error <=  4.779 units, <= 0.33 of its allowance
head            h2          5 cases  bound <=  17.72  floor <=  5.907  kernel error <=  5.907 units, <= 0.33 of its allowance
head            h3          5 cases  bound <=  22.08  floor <=  7.360  kernel error <=  7.360 units, <= 0.33 of its allowance
head            out         5 cases  bound <=   1.66  floor <=  0.554  kernel error <=  0.554 units, <= 0.36 of its allowance
head            extra       1 cases  bound <=   1.00  floor <=  0.000  kernel error <=  0.000 units, <= 0.00 of its allowance
head bwd        delta_out   5 cases  bound <=   2.14  floor <=  0.713  kernel error <=  0.713 units, <= 0.33 of its allowance
head bwd        delta_h3    5 cases  bound <=  12.04  floor <=  4.013  kernel error <=  4.013 units, <= 0.33 of its allowance
head bwd        delta_h2    5 cases  bound <=  10.58  floor <=  3.527  kernel error <=  3.527 units, <= 0.33 of its allowance
head bwd        delta_h1    5 cases  bound <=  14.87  floor <=  4.956  kernel error <=  4.956 units, <= 0.33 of its allowance
head bwd        delta_h0    5 cases  bound <=  11.95  floor <=  3.982  kernel error <=  3.982 units, <= 0.33 of its allowance
head bwd        d_feat      5 cases  bound <=  16.94  floor <=  5.647  kernel error <=  5.647 units, <= 0.33 of its allowance
head bwd        d_normals   5 cases  bound <=   8.61  floor <=  2.870  kernel error <=  2.870 units, <= 0.33 of its allowance
head bwd        d_pts       5 cases  bound <=   9.71  floor <=  3.236  kernel error <=  3.236 units, <= 0.33 of its allowance
head bwd        d_dirs      5 cases  bound <=   9.73  floor <=  3.245  kernel error <=  2.925 units, <= 0.57 of its allowance
head acc        d_feat      5 cases  bound <=   7.95  floor <=  2.651  kernel error <=  2.651 units, <= 0.33 of its allowance
head acc        d_normals   5 cases  bound <=   2.91  floor <=  0.970  kernel error <=  0.970 units, <= 0.33 of its allowance
head acc        d_pts       5 cases  bound <=   2.91  floor <=  0.970  kernel error <=  0.970 units, <= 0.33 of its allowance
head acc        d_dirs      5 cases  bound <=   3.70  floor <=  1.232  kernel error <=  1.232 units, <= 0.40 of its allowance
head bwd        d_extra     1 cases  bound <=   1.99  floor <=  0.665  kernel error <=  0.991 units, <= 0.50 of its allowance
nerf            pe          6 cases  bound <=   1.62  floor <=  0.541  kernel error <=  0.992 units, <= 0.62 of its allowance
nerf            vpe         6 cases  bound <=   1.58  floor <=  0.526  kernel error <=  0.969 units, <= 0.63 of its allowance
nerf            h0          6 cases  bound <=  10.28  floor <=  3.428  kernel error <=  3.428 units, <= 0.33 of its allowance
nerf            h1          6 cases  bound <=  12.66  floor <=  4.221  kernel error <=  4.221 units, <= 0.33 of its allowance
nerf            h2          6 cases  bound <=  15.22  floor <=  5.074  kernel error <=  5.074 units, <= 0.33 of its allowance
nerf            h3          6 cases  bound <=  18.63  floor <=  6.209  kernel error <=  6.209 units, <= 0.33 of its allowance
nerf            h4          6 cases  bound <=  19.70  floor <=  6.568  kernel error <=  6.568 units, <= 0.33 of its allowance
nerf            h5          6 cases  bound <=  20.71  floor <=  6.903  kernel error <=  6.903 units, <= 0.33 of its allowance
nerf            h6          6 cases  bound <=  11.81  floor <=  3.936  kernel error <=  3.936 units, <= 0.33 of its allowance
nerf            h7          6 cases  bound <=  13.05  floor <=  4.350  kernel error <=  4.350 units, <= 0.33 of its allowance
nerf            hv          6 cases  bound <=   9.55  floor <=  3.183  kernel error <=  3.183 units, <= 0.33 of its allowance
nerf            feature     6 cases  bound <=  19.30  floor <=  6.434  kernel error <=  6.434 units, <= 0.33 of its allowance
nerf            density     6 cases  bound <=  18.30  floor <=  6.099  kernel error <=  6.099 units, <= 0.33 of its allowance
nerf            rgb         6 cases  bound <=   6.86  floor <=  2.288  kernel error <=  2.288 units, <= 0.33 of its allowance
nerf            feat        5 cases  bound <=  15.72  floor <=  5.240  kernel error <=  5.240 units, <= 0.33 of its allowance
nerf bwd        delta_o     6 cases  bound <=   1.00  floor <=  0.000  kernel error <=  0.000 units, <= 0.00 of its allowance
nerf bwd        delta_v     6 cases  bound <=  12.93  floor <=  4.311  kernel error <=  4.311 units, <= 0.33 of its allowance
nerf bwd        delta_head  6 cases  bound <=  11.50  floor <=  3.834  kernel error <=  3.834 units, <= 0.33 of its allowance
nerf bwd        delta_h7    6 cases  bound <=  15.17  floor <=  5.058  kernel error <=  5.058 units, <= 0.33 of its allowance
nerf bwd        delta_h6    6 cases  bound <=  11.61  floor <=  3.870  kernel error <=  3.870 units, <= 0.33 of its allowance
nerf bwd        delta_h5    6 cases  bound <=  14.13  floor <=  4.708  kernel error <=  4.708 units, <= 0.33 of its allowance
nerf bwd        delta_h4    6 cases  bound <=  11.68  floor <=  3.893  kernel error <=  3.893 units, <= 0.33 of its allowance
nerf bwd        delta_h3    6 cases  bound <=  11.87  floor <=  3.955  kernel error <=  3.955 units, <= 0.33 of its allowance
nerf bwd        delta_h2    6 cases  bound <=  11.80  floor <=  3.933  kernel error <=  3.933 units, <= 0.33 of its allowance
nerf bwd        delta_h1    6 cases  bound <=  15.80  floor <=  5.268  kernel error <=  5.268 units, <= 0.33 of its allowance
nerf bwd        delta_h0    6 cases  bound <=  11.10  floor <=  3.701  kernel error <=  3.701 units, <= 0.33 of its allowance
nerf bwd        d_pts4      6 cases  bound <=   5.90  floor <=  1.965  kernel error <=  2.434 units, <= 0.69 of its allowance
nerf bwd        d_dirs      6 cases  bound <=   3.84  floor <=  1.281  kernel error <=  1.127 units, <= 0.69 of its allowance
"""
import functools

import numpy as np
import pytest
import torch

from oracle import mlp_cases, mlp_ops
from test_gpu_ray_ops import Bufs, _call, _status, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SDF_NAMES = list(mlp_cases.SDF_CASES) + list(mlp_cases.SDF_F32_CASES)
HEAD_STATES = ("heads", "heads-other", "heads352", "nodpt")
LN2_100 = np.float32(0.0069314718055994529)              # softplus(0) = ln 2 / 100, as float32


def _guards(b):
    b.check(written=())                                  # (the guard bands only; what is finite is asserted plane by plane)


def _rows(c):
    """(rows of the saves, dense ids of those rows, mask of the listed dense points)."""
    n = c["P"] if c["active_idx"] is None else c["n_active"]
    sel = np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:n].astype(np.int64)
    listed = np.zeros(c["P"], bool)
    listed[sel] = True
    return n, sel, listed


def _saved(b, name, n, cols=None):
    """Plane(s) `name` as float64: its first n rows (the rows behind them must still be NaN), columns :cols."""
    a = b.np(name)
    assert np.isnan(a[..., n:, :]).all(), "%s was written behind the last listed row" % name
    return a[..., :n, :cols]


def _dense(b, name, sel, listed, before=None):
    """A per-point output at the listed points; every other point untouched (NaN, or what it held before)."""
    a = b.np(name)
    if before is None:
        assert np.isnan(a[~listed]).all(), "%s of an unlisted point was written" % name
    else:
        assert np.array_equal(a[~listed], np.asarray(before, np.float64)[~listed]), "%s of an unlisted point was written" % name
    return a[sel]


def _work_list(b, a, c):
    if c["active_idx"] is not None:
        a.active_idx, a.n_active = b.inp(c["active_idx"], torch.int32), b.inp(np.asarray([c["n_active"]]), torch.int32)


def _hold(name, res, rows):
    for k, j in res.items():
        line = "%-26s %-9s bound %.2f units (fp32 floor %.3f)  kernel error %.3f units, %.2f of its allowance" % (
            name, k, j["bound"], j["floor"], j["err"], j["used"])
        rows.append(line)
        assert j["ok"], "%s: %d of %d elements outside, first at %s" % (line, j["n_bad"], j["n"], j["worst"])


def _judge(name, models, planes):
    assert set(models) == set(planes), (sorted(models), sorted(planes))
    for k, m in models.items():
        assert planes[k].shape == m["y64"].shape and np.isfinite(planes[k]).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    try:
        _hold(name, mlp_ops.judge_planes(models, planes), rows)
    finally:
        print("\n".join(rows))


@functools.lru_cache(maxsize=None)
def _renderer(state):
    from vdn_train import factory
    st = mlp_cases.head_states(state) if state in HEAD_STATES else mlp_cases.states(state)
    return factory.build_renderer(wdepth=state != "nodpt", device=torch.device(DEV), states=st, precision="fp32",
                                  depth_before_color=state == "heads352")


def _images(net, state):
    img = getattr(_renderer(state), net)._images()
    torch.cuda.synchronize()
    return img


# ---- what the blob holds ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net,state", [("sdf_network", "init"), ("sdf_network", "hot"), ("sdf_network", "silent"), ("color_network", "heads"),
                                       ("depth_network", "heads"), ("nerf", "heads"), ("color_network", "heads352"), ("nerf", "nodpt"),
                                       ("color_network", "heads-other")])
def test_blob_holds_the_operand_weights_fmt0(net, state):
    """vdn_build_images, fmt 0: every chunk of every stream decoded by the documented layout (csrc/mlp_engine.h, F32) equals
    operand_weights(fmt=0) - float32(float32(scale) W_eff[nmap, kmap]), zeros at -1 map entries, the float32 bias block - exactly;
    the rest of the bias block's KiB is zero."""
    from vdn_hip import images, layout
    img = _images(net, state)
    host = mlp_ops.HostImages.of(img)
    assert img.fmt == images.FMT_F32 and img.blobs and "c2" not in img.blobs
    n_chunks = 0
    for sname, blob in img.blobs.items():
        layers = img.streams[sname]
        stride = images.chunk_stride(max(max(L.kt for L in layers), images.STREAM_KT_MAX.get(sname, 0)), images.FMT_F32)
        raw = blob.cpu()
        assert raw.numel() == stride * sum(len(L.chunks) for L in layers)
        off = 0
        for li in range(len(layers)):
            want = mlp_ops.operand_weights(host, sname, li, fmt=0)
            kt = want["kt"]
            for ci in range(want["n_chunks"]):
                chunk = raw[off:off + stride]
                W, bias = layout.decode_chunk_f32(chunk, kt)
                where = "%s %s layer %d chunk %d" % (net, sname, li, ci)
                assert np.array_equal(W.double().numpy(), want["W"][32 * ci:32 * ci + 32]), where
                assert np.array_equal(bias.double().numpy(), want["b"][32 * ci:32 * ci + 32]), where
                assert not chunk[kt * 4096 + 128:kt * 4096 + 1024].any(), where + ": the bias block's padding"
                off += stride
                n_chunks += 1
    assert n_chunks > 20


# ---- the SDF forward --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sdf_images(state):
    """(refreshed NetImages, forward operand weights by layer, the sweep's W_l^T by l, the fbar stream's W_l^T by l, row 0 of W_8)."""
    img = _images("sdf_network", state)
    host = mlp_ops.HostImages.of(img)
    return (img,) + mlp_ops.sdf_ops_f32(host) + (host.weff["lin8"][0].astype(np.float64),)


def _sdf_args(b, c, img, stream):
    from vdn_hip import lib
    a = lib.VdnSdfArgs()
    a.blob = img.blobs[stream].data_ptr()
    a.pts, a.n_per_ray, a.sdf_ld, a.P, a.scale = b.inp(c["pts"]), 1, 1, c["P"], c["scale"]
    a.sdf = b.out("sdf", c["P"])
    _work_list(b, a, c)
    return a


def _sdf_forward_launch(c, state=None):
    """vdn_sdf_mlp_fwd_f32 mode 1 with every save -> (Bufs after the launch, planes {name: float64 rows})."""
    img = _sdf_images(state or c["state"])[0]
    P = c["P"]
    b = Bufs()
    a = _sdf_args(b, c, img, "full")
    a.w8row = img.weff_view("lin8").data_ptr()
    a.normals, a.feat = b.out("normals", P, 3), b.out("feat", P, 256)
    a.S, a.H, a.V, a.PE = b.out("S", 8, P, 256), b.out("H", 8, P, 256), b.out("V", 8, P, 256), b.out("PE", P, 64)
    a.U_pe = b.out("U_pe", P, 39)
    _call("vdn_sdf_mlp_fwd_f32", 1, a, _stream())
    _guards(b)
    n, sel, listed = _rows(c)
    planes = {"PE": _saved(b, "PE", n, 39), "feat": _saved(b, "feat", n), "U_pe": _saved(b, "U_pe", n),
              "sdf": _dense(b, "sdf", sel, listed), "normals": _dense(b, "normals", sel, listed)}
    for k in ("H", "S", "V"):
        full = _saved(b, k, n)
        for l in range(8):
            planes["%s%d" % (k, l)] = full[l]
    return b, planes


@functools.lru_cache(maxsize=None)
def _sdf_forward(name):
    """The forward launch of a case, once: the backward tests run on its device buffers."""
    c = mlp_cases.sdf_case(name)
    return (c,) + _sdf_forward_launch(c)


def _promised(planes):
    """The planes cut to their promised columns (217 of H[3] / S[3] / V[3])."""
    return {k: (v[:, :217] if k in ("H3", "S3", "V3") else v) for k, v in planes.items()}


@pytest.mark.parametrize("name", SDF_NAMES)
def test_sdf_forward_planes_vs_float64_layer_models(name):
    c, _, planes = _sdf_forward(name)
    _, ops, ops_sweep, _, w8row = _sdf_images(c["state"])
    models = mlp_ops.sdf_plane_models_f32(ops, ops_sweep, w8row, mlp_cases.rows_of(c), c["scale"], planes)
    _judge(name, models, _promised(planes))
    # what nmap of lin3 makes of the columns behind its 217 outputs: zero weights and a zero bias in 217..223 - a pre-activation
    # that is exactly 0 -, nothing at all from 224 on
    assert (planes["H3"][:, 217:224] == LN2_100).all() and (planes["S3"][:, 217:224] == 0.5).all() and (planes["V3"][:, 217:224] == 0).all()
    assert all(np.isnan(planes[k][:, 224:]).all() for k in ("H3", "S3", "V3"))
    if c["state"] == "silent":                           # the silenced unit: S = 1/2 on the boundary of a >= 0 ? r : e r
        l, u = mlp_cases.SDF_SILENT
        assert (planes["H%d" % l][:, u] == LN2_100).all() and (planes["S%d" % l][:, u] == 0.5).all()


@pytest.mark.parametrize("name", SDF_NAMES)
def test_sdf_mode0_gives_the_sdf_of_mode1_bit_for_bit(name):
    """vdn_sdf_mlp_fwd_f32 mode 0 (the 'sdf' stream, softplus100_fast) against mode 1 (softplus100_both): the two share the
    expression of h and the k order of every layer, so the sdf is asked to be the same float32."""
    c, _, planes = _sdf_forward(name)
    img = _sdf_images(c["state"])[0]
    b = Bufs()
    a = _sdf_args(b, c, img, "sdf")
    _call("vdn_sdf_mlp_fwd_f32", 0, a, _stream())
    _guards(b)
    _, sel, listed = _rows(c)
    sdf = _dense(b, "sdf", sel, listed)
    assert np.isfinite(sdf).all() and np.array_equal(sdf, planes["sdf"]), np.abs(sdf - planes["sdf"]).max()


def test_the_sdf_launch_on_the_other_weights_is_rejected():
    """The wiring from the launch to the comparator: the same launch on the OTHER state's blob, judged against this state's models,
    is rejected at every plane that depends on a weight matrix (the sdf row of W_8, which also makes V[7], is the geometric init's
    constant in both states; the encoding and its Jacobian have no weights)."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    _, ops, ops_sweep, _, w8row = _sdf_images(c["state"])
    _, planes = _sdf_forward_launch(c, state="other")
    planes = _promised(planes)
    res = mlp_ops.judge_planes(mlp_ops.sdf_plane_models_f32(ops, ops_sweep, w8row, c["pts"], c["scale"], planes), planes)
    assert res["PE"]["ok"] and res["normals"]["ok"]
    for k, j in res.items():
        if k not in ("PE", "normals", "sdf", "V7"):
            assert not j["ok"] and j["err"] > 1e3, (k, j)


# ---- the SDF backward -------------------------------------------------------------------------------------------------------

AB_COLS = (288,) + (256,) * 8


def _blocks(flat, P, cols, n):
    """The row-major blocks of a flat workspace (UB / AB: P-row blocks of the given widths, one behind the other), rows :n."""
    out, off = [], 0
    for w in cols:
        blk = flat[off:off + P * w].reshape(P, w)
        assert np.isnan(blk[n:]).all(), "a block was written behind the last listed row"
        out.append(blk[:n])
        off += P * w
    return out


def _sdf_backward(c, fb, kind, s_from_h, before=None, ex_from=None):
    """rbar then fbar (ex_from: fbar alone on that launch's EX) -> (Bufs, ub blocks, EX planes, ab blocks by layer, d_pts rows)."""
    from vdn_hip import lib
    img = _sdf_images(c["state"])[0]
    P = c["P"]
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    n, sel, listed = _rows(c)
    gf = np.zeros((P, 256), np.float32)
    gf[:n] = g_feat[sel]                                 # (a plane: compact rows, like every save and delta)
    b = Bufs()
    S = fb["H"] if s_from_h else fb["S"]
    fa = lib.VdnSdfFbarArgs()
    pts, gn = b.inp(c["pts"]), b.inp(g_n)
    if ex_from is None:
        rb = lib.VdnSdfRbarArgs()
        rb.blob, rb.pts, rb.n_per_ray, rb.z_ld, rb.P, rb.scale = img.blobs["full"].data_ptr(), pts, 1, 1, P, c["scale"]
        rb.g_normals, rb.S, rb.V, rb.s_from_h = gn, S.data_ptr(), fb["V"].data_ptr(), s_from_h
        rb.UB, rb.EX = b.out("UB", P * 2144), b.out("EX", 8, P, 256)
        _work_list(b, rb, c)
        _call("vdn_sdf_bwd_rbar_f32", rb, _stream())
    fa.blob, fa.g_sdf, fa.g_feat = img.blobs["fbar"].data_ptr(), b.inp(g_sdf), b.inp(gf)
    fa.S, fa.EX, fa.P, fa.scale, fa.s_from_h = S.data_ptr(), (ex_from or b)["EX"].data_ptr(), P, c["scale"], s_from_h
    fa.AB = b.out("AB", P * 2336)
    _work_list(b, fa, c)
    fa.pts, fa.n_per_ray, fa.z_ld, fa.g_normals, fa.U_pe = pts, 1, 1, gn, fb["U_pe"].data_ptr()
    fa.acc_pts, fa.d_pts = int(before is not None), b.out("d_pts", P, 3)
    if before is not None:
        b["d_pts"].copy_(torch.as_tensor(before).to(DEV))
    _call("vdn_sdf_bwd_fbar_f32", fa, _stream())
    _guards(b)
    ab = _blocks(b.np("AB"), P, AB_COLS, n)[::-1]        # (stored ab8, ab7, .. ab0: index by layer)
    d_pts = _dense(b, "d_pts", sel, listed, before)
    if ex_from is not None:
        return b, None, None, ab, d_pts
    return b, _blocks(b.np("UB"), P, mlp_ops.UB_COLS, n), list(_saved(b, "EX", n)), ab, d_pts


SDF_BWD = [(name, "random") for name in SDF_NAMES] + [("uniform-P129-s1", k) for k in mlp_cases.SDF_UPSTREAM[1:]] + \
          [("hot-P300-s1.5", k) for k in mlp_cases.SDF_UPSTREAM[1:]]


@pytest.mark.parametrize("s_from_h", [0, 1])
@pytest.mark.parametrize("name,kind", SDF_BWD)
def test_sdf_backward_blocks_vs_float64_layer_models(name, kind, s_from_h):
    """vdn_sdf_bwd_rbar_f32 then vdn_sdf_bwd_fbar_f32 on the forward's own planes: ub_0 from g_normals, every further UB block and
    EX[l] from the UB block before it (and S[l] or H[l], V[l]), ab_8 from g_feat / g_sdf, every further AB block from the AB block
    after it, d_pts from ab_0, ab_4 and the forward's U_pe. s_from_h = 0: S is the forward's softplus' planes; s_from_h = 1: S points
    at the H planes. Then fbar again with acc_pts = 1 over a finite pre-fill: the same AB blocks bit for bit, d_pts = pre-fill +
    adjoint. With g_normals = 0, UB and EX are exactly zero."""
    c, fb, fplanes = _sdf_forward(name)
    b, ub, EX, ab, d_pts = _sdf_backward(c, fb, kind, s_from_h)
    _, ops, _, ofb, _ = _sdf_images(c["state"])
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    n, sel, _ = _rows(c)
    S = [fplanes["%s%d" % ("H" if s_from_h else "S", l)] for l in range(8)]
    V = [fplanes["V%d" % l] for l in range(8)]
    pts = mlp_cases.rows_of(c)
    models = mlp_ops.sdf_bwd_models_f32(ops, ofb, pts, c["scale"], g_sdf[sel], g_feat[sel], g_n[sel], S, s_from_h, V, ub, EX, ab)
    planes = {"ub0": ub[0][:, :39], "ub4pe": ub[4][:, 224:263], "ab8": ab[8][:, :257], "d_pts": d_pts}
    for l in range(8):
        w = 217 if l == 3 else 256
        planes["ub%d" % (l + 1)], planes["EX%d" % l], planes["ab%d" % l] = ub[l + 1][:, :w], EX[l][:, :w], ab[l][:, :w]
    models["d_pts"] = mlp_ops.sdf_d_pts_model(ofb, pts, c["scale"], g_n[sel], fplanes["U_pe"], ab[0], ab[4], f32=True)
    tag = "%s/%s/s_from_h=%d" % (name, kind, s_from_h)
    _judge(tag, models, planes)
    if kind == "g_normals=0":
        assert all((planes[k] == 0).all() for k in planes if k.startswith(("ub", "EX")))
    before = mlp_cases.sdf_d_pts_prefill(c)
    _, _, _, ab2, d_pts2 = _sdf_backward(c, fb, kind, s_from_h, before=before, ex_from=b)
    for l in range(9):
        w = {8: 257, 3: 217}.get(l, 256)
        assert np.array_equal(ab[l][:, :w], ab2[l][:, :w]), "ab%d differs with acc_pts = 1" % l
    acc = mlp_ops.sdf_d_pts_model(ofb, pts, c["scale"], g_n[sel], fplanes["U_pe"], ab[0], ab[4], f32=True, before=before[sel])
    _judge(tag + "+acc", {"d_pts": acc}, {"d_pts": d_pts2})


# ---- the heads --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _head_images(net, state):
    img = _images(net, state)
    host = mlp_ops.HostImages.of(img)
    return img, [mlp_ops.operand_weights(host, "fwd", l, fmt=0) for l in range(5)], [mlp_ops.operand_weights(host, "bwd", l, fmt=0) for l in range(5)]


def _head_forward_args(b, c, state=None):
    from vdn_hip import lib
    img = _head_images(c["net"], state or c["state"])[0]
    P, d_out = c["P"], c["d_out"]
    a = lib.VdnRenderNetArgs()
    a.blob, a.feat = img.blobs["fwd"].data_ptr(), b.inp(c["feat"])
    a.pts, a.dirs, a.normals, a.n_per_ray = b.inp(c["pts"]), b.inp(c["dirs"]), b.inp(c["normals"]), 1
    a.P, a.d_out, a.squeeze_out = P, d_out, int(c["squeeze"])
    a.out = b.out("out", P, d_out)
    a.save_h, a.save_small = b.out("h", 4, P, 256), b.out("small", P, 64)
    if c["extra"] is not None:
        a.extra, a.save_extra = b.inp(c["extra"]), b.out("extra", P, 96)
    return a


def _head_forward_launch(c, state=None):
    b = Bufs()
    _call("vdn_rendernet_fwd_f32", _head_forward_args(b, c, state), _stream())
    _guards(b)
    planes = {"small": b.np("small")[:, :33], "out": b.np("out")}
    if c["extra"] is not None:
        planes["extra"] = b.np("extra")
    for l in range(4):
        planes["h%d" % l] = b.np("h")[l]
    return b, planes


@functools.lru_cache(maxsize=None)
def _head_forward(name):
    c = mlp_cases.head_case(name)
    return (c,) + _head_forward_launch(c)


def _head_models(c, planes):
    return mlp_ops.head_plane_models(_head_images(c["net"], c["state"])[1], c["pts"], c["dirs"], c["normals"], c["feat"].astype(np.float64),
                                     planes, c["squeeze"], c["d_out"], extra=c["extra"], f32=True)


@pytest.mark.parametrize("name", list(mlp_cases.HEAD_CASES))
def test_head_forward_planes_vs_float64_layer_models(name):
    """vdn_rendernet_fwd_f32 on explicit points and directions with every save: save_small (and save_extra) from the inputs - the
    copied columns exactly -, save_h[0] from the f32 feature vector it was given and its own save_small (and save_extra),
    save_h[1..3] and out from the plane before; a unit whose pre-activation is exactly zero stores 0."""
    c, _, planes = _head_forward(name)
    _judge(name, _head_models(c, planes), planes)
    for l in (0, 2):
        assert (planes["h%d" % l][:, mlp_cases.SILENT_UNIT] == 0).all()


def test_the_head_launch_on_the_other_weights_is_rejected():
    c = mlp_cases.head_case("color-P33")
    _, planes = _head_forward_launch(c, state="heads-other")
    res = mlp_ops.judge_planes(_head_models(c, planes), planes)
    assert res["small"]["ok"]
    for k, j in res.items():
        if k != "small":
            assert not j["ok"] and j["err"] > 1e3, (k, j)


def _d_extra_before(c):
    return np.random.RandomState(11).standard_normal((c["P"], 96)).astype(np.float32)


def _head_backward_args(b, c, fb, acc=None):
    from vdn_hip import lib
    img = _head_images(c["net"], c["state"])[0]
    P, d_out = c["P"], c["d_out"]
    ldo = 96 if d_out == 96 else 32
    a = lib.VdnRenderNetBwdArgs()
    a.blob, a.g_out, a.out, a.save_h = img.blobs["bwd"].data_ptr(), b.inp(mlp_cases.head_upstream(c)), fb["out"].data_ptr(), fb["h"].data_ptr()
    a.delta_out, a.delta_h, a.d_feat = b.out("delta_out", P, ldo), b.out("delta_h", 4, P, 256), b.out("d_feat", P, 256)
    a.d_normals, a.d_pts, a.d_dirs = b.out("d_normals", P, 3), b.out("d_pts", P, 3), b.out("d_dirs", P, 3)
    a.dirs, a.n_per_ray, a.P, a.d_out, a.squeeze_out = b.inp(c["dirs"]), 1, P, d_out, int(c["squeeze"])
    if c["extra"] is not None:                           # (the kernel ADDS d loss / d extra into d_extra)
        a.d_extra = b.out("d_extra", P, 96)
        b["d_extra"].copy_(torch.as_tensor(_d_extra_before(c)).to(DEV))
    if acc is not None:
        a.acc_feat = a.acc_normals = a.acc_pts = 1
        for k in ("d_feat", "d_normals", "d_pts", "d_dirs"):
            b[k].copy_(torch.as_tensor(acc[k]).float().to(DEV))
    return a


def _head_backward(c, fb, acc=None):
    b = Bufs()
    _call("vdn_rendernet_bwd_f32", _head_backward_args(b, c, fb, acc), _stream())
    _guards(b)
    planes = {"delta_out": b.np("delta_out")[:, :c["d_out"]], "d_feat": b.np("d_feat")}
    for l in range(4):
        planes["delta_h%d" % l] = b.np("delta_h")[l]
    for k in ("d_normals", "d_pts", "d_dirs") + (("d_extra",) if c["extra"] is not None else ()):
        planes[k] = b.np(k)
    return planes


@pytest.mark.parametrize("name", list(mlp_cases.HEAD_CASES))
def test_head_backward_planes_vs_float64_layer_models(name):
    """vdn_rendernet_bwd_f32 on the forward's own planes (ReLU' read from the saved planes): delta_out from g_out and out, every
    delta_h from the delta plane after it, d_feat / d_normals / d_pts from the saved delta_h[0], d_dirs through the encoding's
    Jacobian, d_extra (d_feature = 352) added into what it held; the acc_* = 1 forms add into pre-filled targets."""
    c, fb, fplanes = _head_forward(name)
    planes = _head_backward(c, fb)
    ob = _head_images(c["net"], c["state"])[2]
    hs = [fplanes["h%d" % l] for l in range(4)]
    models = mlp_ops.head_bwd_plane_models(ob, mlp_cases.head_upstream(c), fplanes["out"], hs, planes, c["squeeze"], c["d_out"],
                                           d_extra_before=None if c["extra"] is None else _d_extra_before(c).astype(np.float64), f32=True)
    models["d_dirs"] = mlp_ops.head_d_dirs_model(ob, planes["delta_h0"], c["dirs"], f32=True)
    _judge(name, models, planes)
    rs = np.random.RandomState(5)
    pre = {"d_feat": rs.standard_normal((c["P"], 256)).astype(np.float32), "d_normals": rs.standard_normal((c["P"], 3)).astype(np.float32),
           "d_pts": rs.standard_normal((c["P"], 3)).astype(np.float32), "d_dirs": rs.standard_normal((c["P"], 3)).astype(np.float32)}
    added = _head_backward(c, fb, acc=pre)
    for k in ("delta_out", "delta_h0", "delta_h1", "delta_h2", "delta_h3"):
        assert np.array_equal(planes[k], added[k]), k
    acc_models = {}
    for k in pre:
        m = models[k]
        y64 = m["y64"] + pre[k]
        acc_models[k] = dict(y64=y64, y32=mlp_ops.f32_rne(m["y32"] + pre[k]), unit=m["unit"] + mlp_ops.U24 * np.abs(y64), extra=m["extra"],
                             stored="f32")
    _judge(name + "+acc", acc_models, {k: added[k] for k in pre})


# ---- the background network ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _nerf_images(state):
    img = _images("nerf", state)
    host = mlp_ops.HostImages.of(img)
    return img, [mlp_ops.operand_weights(host, "fwd", l, fmt=0) for l in range(11)], [mlp_ops.operand_weights(host, "bwd", l, fmt=0) for l in range(11)]


def _nerf_forward_args(b, c, state=None):
    from vdn_hip import lib
    img = _nerf_images(state or c["state"])[0]
    P = c["P"]
    a = lib.VdnNerfArgs()
    a.blob, a.pts4, a.dirs, a.n_per_ray, a.P = img.blobs["fwd"].data_ptr(), b.inp(c["pts4"]), b.inp(c["dirs"]), 1, P
    a.density, a.rgb = b.out("density", P), b.out("rgb", P, 3)
    if c["state"] != "nodpt":
        a.feat = b.out("feat", P, 96)
    a.save_h, a.save_pe, a.save_feature = b.out("h", 8, P, 256), b.out("pe", P, 96), b.out("feature", P, 256)
    a.save_vpe, a.save_hv = b.out("vpe", P, 32), b.out("hv", P, 128)
    _work_list(b, a, c)
    return a


def _nerf_forward_launch(c, state=None):
    b = Bufs()
    _call("vdn_nerf_mlp_fwd_f32", _nerf_forward_args(b, c, state), _stream())
    _guards(b)
    n, sel, listed = _rows(c)
    planes = {"pe": _saved(b, "pe", n, 84), "vpe": _saved(b, "vpe", n, 27), "feature": _saved(b, "feature", n), "hv": _saved(b, "hv", n)}
    h = _saved(b, "h", n)
    for l in range(8):
        planes["h%d" % l] = h[l]
    for k in ("density", "rgb") + (("feat",) if c["state"] != "nodpt" else ()):
        planes[k] = _dense(b, k, sel, listed)
    return b, planes


@functools.lru_cache(maxsize=None)
def _nerf_forward(name):
    c = mlp_cases.nerf_case(name)
    return (c,) + _nerf_forward_launch(c)


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_forward_planes_vs_float64_layer_models(name):
    """vdn_nerf_mlp_fwd_f32 on explicit points and directions with every save (with the dpt head; once with a work list: saves in
    compact rows, outputs at the dense positions; once without the dpt head): save_pe / save_vpe from the inputs, every other plane
    and output from the planes before it; the unit whose pre-activation is exactly zero."""
    c, _, planes = _nerf_forward(name)
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    models = mlp_ops.nerf_plane_models(_nerf_images(c["state"])[1], pts4, dirs, planes, f32=True)
    assert ("feat" in planes) == (c["state"] != "nodpt")
    _judge(name, models, planes)
    assert (planes["h2"][:, mlp_cases.SILENT_UNIT] == 0).all()


def test_the_background_launch_on_the_other_weights_is_rejected():
    c = mlp_cases.nerf_case("nerf-P33")
    _, planes = _nerf_forward_launch(c, state="heads-other")
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    res = mlp_ops.judge_planes(mlp_ops.nerf_plane_models(_nerf_images(c["state"])[1], pts4, dirs, planes, f32=True), planes)
    assert res["pe"]["ok"] and res["vpe"]["ok"]
    for k, j in res.items():
        if k not in ("pe", "vpe"):
            assert not j["ok"] and j["err"] > 1e3, (k, j)


def _nerf_backward_args(b, c, fb):
    from vdn_hip import lib
    img = _nerf_images(c["state"])[0]
    P = c["P"]
    g_density, g_rgb, g_feat = mlp_cases.nerf_upstream(c)
    a = lib.VdnNerfBwdArgs()
    a.blob, a.g_density, a.g_rgb, a.g_feat = img.blobs["bwd"].data_ptr(), b.inp(g_density), b.inp(g_rgb), b.inp(g_feat)
    a.save_h, a.save_hv, a.P, a.n_per_ray = fb["h"].data_ptr(), fb["hv"].data_ptr(), P, 1
    ldo = 128 if g_feat is not None else 32
    a.delta_o, a.delta_v = b.out("delta_o", P, ldo), b.out("delta_v", P, 128)
    a.delta_head, a.delta_h = b.out("delta_head", P, 288), b.out("delta_h", 8, P, 256)
    _work_list(b, a, c)
    return a


def _nerf_input_args(b, c):
    from vdn_hip import lib
    ig = lib.VdnNerfInputGradArgs()
    ig.pts4, ig.dirs, ig.accumulate = b.inp(c["pts4"]), b.inp(c["dirs"]), 0
    ig.d_pts4, ig.d_dirs = b.out("d_pts4", c["P"], 4), b.out("d_dirs", c["P"], 3)
    return ig


def _nerf_backward(c, fb, input_adjoint=False):
    b = Bufs()
    a = _nerf_backward_args(b, c, fb)
    if input_adjoint:                                    # (explicit inputs: rows by the dense point id)
        _call("vdn_nerf_mlp_bwd_input_f32", a, _nerf_input_args(b, c), _stream())
    else:
        _call("vdn_nerf_mlp_bwd_f32", a, _stream())
    _guards(b)
    n, sel, listed = _rows(c)
    planes = {"delta_o": _saved(b, "delta_o", n), "delta_v": _saved(b, "delta_v", n), "delta_head": _saved(b, "delta_head", n, 257)}
    dh = _saved(b, "delta_h", n)
    for l in range(8):
        planes["delta_h%d" % l] = dh[l]
    if input_adjoint:
        for k in ("d_pts4", "d_dirs"):
            planes[k] = _dense(b, k, sel, listed)
    return planes


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_backward_planes_vs_float64_layer_models(name):
    """vdn_nerf_mlp_bwd_f32 on the forward's own planes (ReLU' read from the saved planes; with and without the dpt head, with a
    work list: g_* at the dense positions, deltas in compact rows): delta_o from the upstream gradients, delta_v, delta_head and
    delta_h[7..0] each from the delta plane after it."""
    c, fb, fplanes = _nerf_forward(name)
    planes = _nerf_backward(c, fb)
    _, sel, _ = _rows(c)
    g = [None if x is None else x[sel] for x in mlp_cases.nerf_upstream(c)]
    ob = _nerf_images(c["state"])[2]
    models = mlp_ops.nerf_bwd_plane_models(ob, *g, [fplanes["h%d" % l] for l in range(8)], fplanes["hv"], planes, f32=True)
    _judge(name, models, planes)


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_input_adjoint_vs_float64_models(name):
    """vdn_nerf_mlp_bwd_input_f32: the delta planes, and d_pts4 / d_dirs = the encodings' Jacobians on the adjoints of the encoded
    inputs, modelled from the saved delta_h0, delta_h5 and delta_v."""
    c, fb, fplanes = _nerf_forward(name)
    planes = _nerf_backward(c, fb, input_adjoint=True)
    _, sel, _ = _rows(c)
    g = [None if x is None else x[sel] for x in mlp_cases.nerf_upstream(c)]
    ob = _nerf_images(c["state"])[2]
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    models = mlp_ops.nerf_bwd_plane_models(ob, *g, [fplanes["h%d" % l] for l in range(8)], fplanes["hv"], planes, f32=True)
    models.update(mlp_ops.nerf_input_adjoint_models(ob, pts4, dirs, planes, f32=True))
    _judge(name, models, planes)


# ---- what the fp32 entry points refuse ----------------------------------------------------------------------------------------

def _untouched(b):
    torch.cuda.synchronize()
    b.check(unwritten=tuple(b.outs))


def test_the_fp32_entry_points_refuse_the_relu_masks_and_write_nothing():
    """The 1-bit ReLU masks are the bf16 path's: vdn_rendernet_fwd_f32 returns -4 for save_mask and vdn_rendernet_bwd_f32 -5 for
    mask; vdn_nerf_mlp_fwd_f32 -2 for save_mask / save_mask_v, vdn_nerf_mlp_bwd_f32 and vdn_nerf_mlp_bwd_input_f32 -5 for mask /
    mask_v. Nothing is launched: every output still holds its NaN pre-fill."""
    dummy = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)      # (large enough for any mask plane, were one written)
    c, fb, _ = _head_forward("color-P33")
    b = Bufs()
    a = _head_forward_args(b, c)
    a.save_mask = dummy.data_ptr()
    assert _status("vdn_rendernet_fwd_f32", a, _stream()) == -4
    _untouched(b)
    b = Bufs()
    a = _head_backward_args(b, c, fb)
    a.mask = dummy.data_ptr()
    assert _status("vdn_rendernet_bwd_f32", a, _stream()) == -5
    _untouched(b)
    c, fb, _ = _nerf_forward("nerf-P33")
    for fields in (("save_mask",), ("save_mask_v",), ("save_mask", "save_mask_v")):
        b = Bufs()
        a = _nerf_forward_args(b, c)
        for f in fields:
            setattr(a, f, dummy.data_ptr())
        assert _status("vdn_nerf_mlp_fwd_f32", a, _stream()) == -2
        _untouched(b)
    for fields in (("mask",), ("mask_v",), ("mask", "mask_v")):
        b = Bufs()
        a = _nerf_backward_args(b, c, fb)
        for f in fields:
            setattr(a, f, dummy.data_ptr())
        assert _status("vdn_nerf_mlp_bwd_f32", a, _stream()) == -5
        _untouched(b)
        b = Bufs()
        a = _nerf_backward_args(b, c, fb)
        for f in fields:
            setattr(a, f, dummy.data_ptr())
        assert _status("vdn_nerf_mlp_bwd_input_f32", a, _nerf_input_args(b, c), _stream()) == -5
        _untouched(b)
    assert not dummy.any()
