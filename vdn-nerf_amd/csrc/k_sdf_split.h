// What the three "feature-split" kernels of the bf16 SDF network share (gfx950): k_sdf_fwd0_split.h (sdf0s: the sampler's sdf-only
// passes), k_sdf_fwd1_split.h (sdf1s: the tail rows of the training forward) and k_sdf_bwd_split.h (sdfbs: rbar + fbar in one launch).
// One workgroup = 32 rows, 8 waves, wave w owns output tile w (32 features) of every layer step - 16 MFMAs per wave per step; the
// activations meet in LDS between steps (B-fragment order, ping-pong buffers, one barrier per step) and the weights never touch
// LDS: the chunk of (step, tile) is read by exactly one wave, whose lane (i,h) wants the chunk's 16 bytes [k-step][lane] as they
// lie (mlp_engine.h, BF16 chunk format), two steps ahead, into one of two register sets (even / odd steps).
//
// Each of these pieces exists once, here: the barrier, the register set, the MMA step, and - for the two forward kernels, which walk
// the large kernel's (k_sdf_fwd2.h) step list - the LDS map, the step's input / output places, the wave's tile and the pointer-form
// weight load. The kernels keep their own prologues and epilogues (profiles/README.md, "Shared header of the feature-split kernels":
// moving those changed the generated code).
#pragma once
#include "k_sdf_fwd2.h"

namespace vdn {
namespace split {

constexpr int kWaves = 8;

VDN_DEV void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// this wave's A fragments of one step (at most 9 input tiles = 18 k-steps) and, where the step has one, its bias rows
struct WSet {
    bf16x8 w[18];
    f32x4 b[4];
};

// One MMA step of a wave: acc = (bias | 0) + W . X over IO::ns k-steps; IO::in_off(s) = LDS byte offset of k-step s of the input.
// PRE B fragments are read up front, then one read per MFMA (mlp_engine.h, BF16::mma).
// PRE_MAX: 6 in the forward kernels, 4 in the backward (k_sdf_bwd_split.h: 6 makes no difference there and costs 8 registers).
template <class IO, int PRE_MAX, bool BIAS>
VDN_DEV f32x16 step_mma(const WSet& W, const char* smem, int lane) {
    constexpr int NS = IO::ns;
    constexpr int PRE = NS < PRE_MAX ? NS : PRE_MAX;
    f32x16 acc;
    if constexpr (BIAS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[4 * q + 0] = W.b[q][0]; acc[4 * q + 1] = W.b[q][1]; acc[4 * q + 2] = W.b[q][2]; acc[4 * q + 3] = W.b[q][3];
        }
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = 0.0f;
    }
    bf16x8 x[NS];
    static_for<NS>([&](auto s_c) VDN_INL {
        constexpr int s = decltype(s_c)::value;
        x[s] = *reinterpret_cast<const bf16x8*>(smem + IO::in_off(s) + lane * 16);
    });
    static_for<NS>([&](auto s_c) VDN_INL {
        constexpr int s = decltype(s_c)::value;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W.w[s], x[s], acc, 0, 0, 0);
    });
    __builtin_amdgcn_sched_group_barrier(0x100, PRE, 0);
    static_for<NS - PRE>([&](auto) VDN_INL {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    });
    __builtin_amdgcn_sched_group_barrier(0x008, PRE, 0);
    return acc;
}

// ---- the forward kernels (PG = sdf2::Prog<0> or sdf2::Prog<1>: the large kernel's weight stream and step list) ------------------
constexpr int kPeb = 0;                         // encoded input, 4 k-steps x 1 KiB (layer 0's input; k-steps 14..17 of layer 4)
constexpr int kBuf0 = 4 * 1024;                 // activations, 16 k-steps x 1 KiB each, ping-pong
constexpr int kBuf1 = kBuf0 + 16 * 1024;
constexpr int kW8 = kBuf1 + 16 * 1024;          // row 0 of the last layer, 256 f32
constexpr int kG = kW8 + 1024;                  // layer 7's activations in f32: [tile][q][lane] x 16 B (the f32 sdf row)
constexpr int kFwdLds = kG + 8 * 4 * 1024;

template <class PG, int LI>
struct FwdIO {
    static constexpr sdf2::LayerDesc L = PG::layer(LI);
    static constexpr int kt = L.kt, nt = L.nt, ns = 2 * L.kt;
    // LDS byte offset of k-step s of step LI's input
    static constexpr int in_off(int s) {
        if (LI == 0) return kPeb + s * 1024;
        if (LI == 4 && s >= 14) return kPeb + (s - 14) * 1024;
        return ((LI & 1) ? kBuf0 : kBuf1) + s * 1024;           // step LI-1 wrote buffer (LI-1) & 1
    }
    static constexpr int out_base = (LI & 1) ? kBuf1 : kBuf0;
    static constexpr bool bias = L.kind <= sdf2::LAST;
};

// the tile wave w computes in step LI: its own where the step has it (layer 3 has 7: wave 7 recomputes tile 6 and drops it);
// the two encoding tiles of the skip layer's sweep (7, then 8) and of W0^T (0, then 1) are wave 7's
template <class PG, int LI>
VDN_DEV int tile_of_wave(int wave) {
    constexpr int nt = PG::layer(LI).nt;
    if constexpr (PG::layer(LI).kind == sdf2::SWEEP_PE) return 0;
    if constexpr (PG::layer(LI).kind == sdf2::SWEEP_SKIP) return wave;           // 0..7 (tile 8 follows on wave 7)
    return wave < nt ? wave : nt - 1;
}

// the chunk of (step LI, tile) -> registers
template <class PG, int LI>
VDN_DEV void load_weights(WSet& W, const char* blob, int tile, int lane) {
    using IO = FwdIO<PG, LI>;
    const char* ch = blob + (long)(PG::first_chunk(LI) + tile) * sdf2::kStride;
    const bf16x8* wa = reinterpret_cast<const bf16x8*>(ch) + lane;
    static_for<IO::ns>([&](auto s_c) VDN_INL { W.w[decltype(s_c)::value] = wa[decltype(s_c)::value * 64]; });
    if constexpr (IO::bias) {
        const f32x4* bb = reinterpret_cast<const f32x4*>(ch + IO::kt * 2048);
#pragma unroll
        for (int q = 0; q < 4; ++q) W.b[q] = bb[2 * q + (lane >> 5)];
    }
}

}  // namespace split
}  // namespace vdn
