// The flat weight-stream pipeline of the bf16 kernels, once: the fused SDF kernel (k_sdf_fwd2.h) and the flat-stream engine
// (mlp_flow.h) both run on it. A kernel's weight stream is a sequence of chunks (mlp_engine.h's chunk format, BF16 policy, uniform
// stride); a ring of LDS slots is filled by LDS-DMA, and chunk step c
//   * issues chunk c's MFMAs from fragments read kPre MFMAs ahead (the opening ones by step c-1, across the chunk boundary);
//   * behind its first MFMA group certifies chunk c+1: a counted s_waitcnt vmcnt(N) for this wave's pieces, then the workgroup
//     barrier for the other waves' - the barrier is off the MFMA path;
//   * issues the DMA pieces of chunk c+DEPTH into the slot chunk c-1 was read from (every wave is past the barrier);
//   * hands every MFMA group to the caller's VALU work (the epilogue of chunk c-1's tile runs in the shadow of chunk c's MFMAs);
//   * reloads the bias rows of chunk c+1 in its last group.
// The ordering rules live here and nowhere else: nothing but counted vector-memory operations may be younger than a DMA (every
// lane issues every counted load / store, so all wait counts are compile-time constants - which operations those are follows from
// the user's issue order and is its policy's wait()), and a DMA may only overwrite a slot that every wave has left at the latest barrier.
// LDS-DMA is inline asm: the builtin makes hipcc's wait-count pass treat every later LDS wait as out of order (it marks a pending
// FLAT access), and it then emits s_waitcnt lgkmcnt(0) in front of every MFMA that consumes a fragment - a full LDS round trip per
// MFMA group instead of a counted wait. The compiler does not see these loads: its own LDS waits stay counted, and its waits for
// ordinary loads count only what it knows (which can only wait longer, never shorter).
//
// What differs between the users is a compile-time POLICY:
//   static constexpr int total;                      chunks in the stream
//   static constexpr int kt(int c);                  k-tiles of chunk c (0 beyond the stream)
//   static constexpr bool bias(int c);               chunk c initialises its accumulator from its bias block
//   static constexpr bool certifies(int c);          step c waits and synchronises for the chunk(s) behind it
//   static constexpr int wait(int c);                the vmcnt immediate of that wait (derived from the user's issue order)
//   static constexpr bool dma_burst(int c);          step c issues its DMA pieces in one burst behind the barrier (else one per group)
//   static constexpr int kPre, kGroup;               fragments read ahead of their MFMA (the pipe's PRE); MFMAs per scheduling group
#pragma once
#include "mlp_engine.h"

namespace vdn {
namespace cstream {

template <int N>
VDN_DEV void wait_vmcnt() {
    static_assert(N >= 0 && N <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// accumulator registers 4 g .. 4 g + 3 of a lane are features 4 quad_of(g) .. + 3 of the tile's natural order
VDN_DEV int quad_of(int g, int lane) { return 2 * g + (lane >> 5); }
// the accumulator of a chunk step (v_mfma_f32_32x32x16_bf16): lane = c + 32 h owns point c; register t = feature (t&3) + 8 (t>>2) + 4 h
// (vdn_common.h)
struct Acc32 {
    f32x16 w;
    VDN_DEV float operator[](int t) const { return w[t]; }
    VDN_DEV void fill(const f32x4 (&bias)[4], bool with_bias) {
#pragma unroll
        for (int t = 0; t < 16; ++t) w[t] = with_bias ? bias[t >> 2][t & 3] : 0.0f;
    }
    template <int S, class ActT>
    VDN_DEV void mfma(const bf16x8& a, const ActT& X) { w = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, X.r[S], w, 0, 0, 0); }
};

constexpr int kNoSplit = 1 << 30;

// ---- pipeline state ---------------------------------------------------------------------------------------------
// NWAVES waves share a ring of NSLOT slots of STRIDE bytes, DEPTH chunks in flight; chunks from SPLIT on come from a second
// stream (without one, g2 is never read and costs nothing)
template <int NWAVES, int STRIDE, int NSLOT, int DEPTH, int SPLIT = kNoSplit, int PRE = 4>
struct Pipe {
    static_assert(STRIDE % (1024 * NWAVES) == 0, "chunk stride must be a multiple of NWAVES KiB");
    static_assert(NSLOT >= DEPTH + 1, "ring: the chunk being read, the one being opened and DEPTH-1 in flight");
    static constexpr int kG = STRIDE / 1024 / NWAVES;     // DMA instructions (1-KiB pieces) per wave per chunk
    static constexpr int kDepth = DEPTH, kSlots = NSLOT, kPre = PRE;
    const char* g;      // weight stream (wave-uniform)
    const char* g2;     // chunks from SPLIT on: the second stream
    char* lds;          // ring base
    int wave, lane;
    bf16x8 fr[PRE];     // opening fragments of the next chunk step (already read)
    f32x4 bias[4];      // its bias rows
    unsigned voff0;     // lane * 16 + this wave's first byte in a chunk + 4096 (the centre of the pieces' immediate offsets)
    unsigned m0_wave;   // LDS byte address of the same place in ring slot 0
    VDN_DEV void init(const char* blob, char* smem, const char* blob2 = nullptr) {
        g = blob;
        g2 = blob2;
        lds = smem;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        lane = threadIdx.x & 63;
        voff0 = lane * 16 + wave * (kG * 1024) + 4096;
        m0_wave = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds + wave * (kG * 1024) + 4096);
    }
    // (the dump area of the warm-up's LDS-DMA: this wave's own first piece of ring slot 0 - vdn_common.h)
    VDN_DEV char* warm_dump() const { return lds + wave * (kG * 1024); }
    template <int C>
    VDN_DEV char* slot() const { return lds + (C % NSLOT) * STRIDE; }
    // DMA piece I (of kG) of chunk C: 1 KiB, wave-uniform base + per-lane 32-bit offset + immediate; one M0 write per chunk, by
    // piece 0 (vdn_common.h: glds16_imm*)
    template <int C, int I>
    VDN_DEV void issue_piece() {
        constexpr long COFF = (C >= SPLIT ? (long)(C - SPLIT) : (long)C) * STRIDE;
        const char* base = C >= SPLIT ? g2 : g;
        static_assert(kG <= 8, "one group of immediate offsets");
        static_assert(COFF + STRIDE < (1L << 31), "32-bit chunk offsets");
        const unsigned voff = voff0 + (unsigned)COFF;
        if constexpr (I == 0) glds16_imm_m0add<(C % NSLOT) * STRIDE, glds_imm(I)>(base, voff, m0_wave);
        else glds16_imm<glds_imm(I)>(base, voff);
    }
    template <int C>
    VDN_DEV void issue() {
        static_for<kG>([&](auto i_c) VDN_INL { issue_piece<C, decltype(i_c)::value>(); });
    }
    VDN_DEV void load_bias(const f32x4* b) {
#pragma unroll
        for (int q = 0; q < 4; ++q) bias[q] = b[quad_of(q, lane)];
    }
    // reads that open chunk step C (its first fragments, and its bias rows)
    template <class PL, int C>
    VDN_DEV void prefetch() {
        constexpr int KT = PL::kt(C);
        const char* w = slot<C>();
        const bf16x8* wa = reinterpret_cast<const bf16x8*>(w) + lane;
#pragma unroll
        for (int s = 0; s < (PRE < 2 * KT ? PRE : 2 * KT); ++s) fr[s] = wa[s * 64];
        if constexpr (PL::bias(C)) load_bias(reinterpret_cast<const f32x4*>(w + KT * 2048));
    }
    // ring start: chunks 0 .. DEPTH-1 in flight, chunk 0 certified, its opening fragments read. Call it behind every ordinary
    // load / store of the prologue (nothing but counted operations may be younger than a DMA): it drains them first.
    template <class PL>
    VDN_DEV void start() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        static_for<DEPTH>([&](auto c_c) VDN_INL {
            constexpr int C = decltype(c_c)::value;
            if constexpr (C < PL::total) issue<C>();
        });
        wait_vmcnt<(DEPTH - 1 < PL::total - 1 ? DEPTH - 1 : PL::total - 1) * kG>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        prefetch<PL, 0>();
    }
};

// One chunk step: acc = (bias) + W[chunk C] . X over kt(C) input tiles. group(gi, NG) = the VALU work assigned to MFMA group gi
// of NG (kGroup MFMAs per group). Group 0 certifies; the DMA pieces of chunk C+DEPTH follow (in a burst, or one per group); the
// tail reads the opening fragments of chunk C+1.
template <class PL, int C, class PipeT, class ActT, class Group>
VDN_DEV Acc32 chunk_step(PipeT& pp, const ActT& X, Group&& group) {
    static_assert(PL::kPre == PipeT::kPre, "the pipe holds the opening fragments");
    constexpr int kPre = PL::kPre, kGroup = PL::kGroup, kG = PipeT::kG, DEPTH = PipeT::kDepth;
    constexpr int KT = PL::kt(C);
    constexpr int NS = KT * 2, NG = (NS + kGroup - 1) / kGroup;
    constexpr int KTN = PL::kt(C + 1);
    constexpr bool HAS_NEXT = C + 1 < PL::total;
    constexpr bool HAS_DMA = C + DEPTH < PL::total;
    const bf16x8* wa = reinterpret_cast<const bf16x8*>(pp.template slot<C>()) + pp.lane;
    const bf16x8* wn = reinterpret_cast<const bf16x8*>(pp.template slot<C + 1>()) + pp.lane;
    bf16x8 fr[NS];
    Acc32 acc;
    constexpr int PF = kPre < NS ? kPre : NS;                       // fragments of this chunk read by the previous step
    constexpr int PFN = kPre < 2 * KTN ? kPre : 2 * KTN;            // fragments of the next chunk this step reads
    static_for<PF>([&](auto s_c) VDN_INL { fr[decltype(s_c)::value] = pp.fr[decltype(s_c)::value]; });
    acc.fill(pp.bias, PL::bias(C));
    __builtin_amdgcn_sched_barrier(0);
    static_for<NG>([&](auto g_c) VDN_INL {
        constexpr int gi = decltype(g_c)::value;
        constexpr int s0 = gi * kGroup, s1 = (gi + 1) * kGroup < NS ? (gi + 1) * kGroup : NS;
        static_for<s1 - s0>([&](auto j_c) VDN_INL {
            constexpr int s = s0 + decltype(j_c)::value;
            acc.template mfma<s>(fr[s], X);
        });
        if constexpr (gi == 0 && HAS_NEXT && PL::certifies(C)) {
            __builtin_amdgcn_sched_barrier(0);      // the step's first MFMAs are in the pipe while the wave waits
            wait_vmcnt<PL::wait(C)>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
        // DMA of chunk C+DEPTH (into the slot chunk C-1 was read from: every wave is past the barrier): all pieces right behind
        // the barrier, or spread over the groups
        if constexpr (HAS_DMA && PL::dma_burst(C)) {
            if constexpr (gi == 0) pp.template issue<C + DEPTH>();
        } else if constexpr (HAS_DMA) {
            static_for<kG>([&](auto i_c) VDN_INL {
                constexpr int i = decltype(i_c)::value;
                if constexpr ((NG >= kG ? i * NG / kG : (i < NG ? i : NG - 1)) == gi) pp.template issue_piece<C + DEPTH, i>();
            });
        }
        // fragment reads kPre MFMAs ahead: the rest of this chunk, then the opening fragments of chunk C+1
        static_for<s1 - s0>([&](auto j_c) VDN_INL {
            constexpr int s = s0 + decltype(j_c)::value;
            if constexpr (s + PF < NS) fr[s + PF] = wa[(s + PF) * 64];
            else if constexpr (HAS_NEXT && s + PF - NS < PFN) pp.fr[s + PF - NS] = wn[(s + PF - NS) * 64];
            // a chunk shorter than the next one's opening: its last MFMA slot reads the remainder
            if constexpr (HAS_NEXT && s == NS - 1)
                static_for<(PFN > PF ? PFN - PF : 0)>([&](auto e_c) VDN_INL { pp.fr[PF + decltype(e_c)::value] = wn[(PF + decltype(e_c)::value) * 64]; });
        });
        if constexpr (gi == NG - 1 && HAS_NEXT && KTN > 0 && PL::bias(C + 1)) {
            pp.load_bias(reinterpret_cast<const f32x4*>(pp.template slot<C + 1>() + KTN * 2048));
        }
        group(g_c, std::integral_constant<int, NG>{});
        __builtin_amdgcn_sched_barrier(0);
    });
    return acc;
}

}  // namespace cstream
}  // namespace vdn
