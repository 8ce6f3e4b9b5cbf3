// Flat-stream MLP engine for the bf16 kernels (round 2): the chunk-stream pipeline of k_sdf_fwd2.h (chunk_stream.h: the ring, the
// LDS-DMA, the counted waits, the chunk step) behind the interface of mlp_engine.h's dense(), for the colour / VDN heads and the
// background network (forward and backward chains).
//
//   * a kernel's weight stream is a compile-time PROGRAM: for every 32-row chunk its contraction width (k-tiles), whether it
//     carries a bias block, and how many vector-memory instructions its tile's pre() (loads) and epi() (stores) issue;
//   * chunk step c runs the epilogue of chunk c-1's tile under chunk c's MFMAs (also across layer boundaries: before the MFMA
//     group that reads the pending tile): the matrix pipe streams across chunk and layer boundaries, no drain steps;
//   * every step certifies chunk c+1 and issues all DMA pieces of chunk c+DEPTH in one burst behind the barrier;
//   * every wait count is a compile-time constant: every lane issues every plane load / store (out-of-range lanes work on a
//     clamped row: loads read it, stores write duplicates of it).
//
// The chunk index and the pending epilogue travel in the TYPE of the flow object: dense2() takes Flow<C, Pend> and returns
// Flow<C + NT, Pending<Epi, Aux>>; flow_finish() runs the last pending epilogue.
#pragma once
#include <type_traits>
#include "chunk_stream.h"

namespace vdn {
namespace flow {

constexpr int kPre = 4;        // weight fragments read ahead of their MFMA
constexpr int kGroup = 2;      // MFMAs per scheduling group

template <int NWAVES, int STRIDE, int NSLOT, int DEPTH>
using Pipe = cstream::Pipe<NWAVES, STRIDE, NSLOT, DEPTH, cstream::kNoSplit, kPre>;

// A program: struct with
//   static constexpr int total;                      chunks in the stream
//   static constexpr int kt(int c);                  k-tiles of chunk c (0 beyond the stream)
//   static constexpr bool bias(int c);               chunk c initialises its accumulator from its bias block
//   static constexpr int loads(int c);               vector-memory loads pre() issues for chunk c's tile (in step c)
//   static constexpr int stores(int c);              vector-memory stores epi() issues for chunk c's tile (in step c+1)
//   static constexpr bool drained(int c);            the kernel runs chunk c's epilogue right behind step c (flow_drain)

// The engine's policy of the chunk step (chunk_stream.h): the program PG on a pipe PipeT, every step certifies, every DMA is a burst
template <class PG, class PipeT>
struct Policy : PG {
    static constexpr int kPre = flow::kPre, kGroup = flow::kGroup;
    static constexpr bool certifies(int) { return true; }
    static constexpr bool dma_burst(int) { return true; }
    // s_waitcnt vmcnt(N) that retires this wave's DMA of chunk c+1 in step c, before its barrier. Step j issues, in order: the
    // loads of pre(j); [its first MFMAs; the wait; the barrier]; ALL DMA pieces of chunk j+DEPTH; then the stores of epi(j-1).
    // (The DMA goes first on purpose: vmcnt retires in issue order, so a store issued BEFORE the awaited DMA would have to be
    // acknowledged by memory before the wait returns - every step would pay an HBM write round trip.) Younger than DMA(c+1),
    // issued in step c+1-DEPTH, are therefore: that step's stores, everything of steps c+2-DEPTH .. c-1, and the loads of pre(c).
    static constexpr int wait(int c) {
        constexpr int DEPTH = PipeT::kDepth;
        int n = PG::loads(c);
        for (int j = c + 1 - DEPTH; j <= c - 1; ++j) {
            if (j < 0) continue;
            // the stores of epi(j-1) run in step j behind its DMA - unless the kernel drained that epilogue at the end of step
            // j-1 (flow_drain): then they are OLDER than step j's DMA and must not be counted (a count too large releases the
            // wait while DMA pieces are still in flight)
            if (!PG::drained(j - 1)) n += PG::stores(j - 1);
            if (j >= c + 2 - DEPTH) {
                n += PG::loads(j);
                if (j + DEPTH < PG::total) n += PipeT::kG;
            }
        }
        return n < 63 ? n : 63;
    }
};

struct NoPend {
    static constexpr int tile = -1;
    VDN_DEV void run() const {}
};
// the epilogue of a chunk's tile, waiting to run under the next chunk's MFMAs
template <class Epi, class Aux, int TILE = -1>
struct Pending {
    static constexpr int tile = TILE;       // the output tile it belongs to (known once it is a layer's last tile)
    Epi epi;
    f32x16 acc;
    Aux aux;
    int nt;
    VDN_DEV void run() const { epi(nt, acc, aux); }
};

template <int C, class Pend>
struct Flow {
    Pend pend;
};

// the step's group callback that runs `mid` once, in group min(G_EPI, NG - 1): the group chosen for the pending epilogue
template <int G_EPI, class Mid>
VDN_DEV auto in_group(Mid mid) {
    return [mid](auto g_c, auto ng_c) VDN_INL {
        constexpr int NG = decltype(ng_c)::value;
        if constexpr (decltype(g_c)::value == (G_EPI < NG ? G_EPI : NG - 1)) mid();
    };
}

// One dense layer on the wave's 32 points: for every output tile nt, acc = bias + W[nt] . X, then epi(nt, acc, aux) with
// aux = pre(nt) (its loads are issued at the top of the tile's chunk step, one step before epi consumes them).
//   WRITES_INPUT: this layer's epilogue writes the activation tile nt of the NEXT layer's input (so, across the layer boundary,
//   it has to complete before the MFMA group that reads k-steps 2 nt, 2 nt + 1).
// Returns the flow advanced by NT chunks, carrying this layer's last tile as the pending epilogue.
template <class PG, int NT, bool PREV_WRITES_INPUT = true, int C, class PendIn, class PipeT, class ActT, class Pre, class Epi>
VDN_DEV auto dense2(Flow<C, PendIn> f, PipeT& pp, const ActT& X, Pre&& pre, Epi&& epi) {
    using EpiT = std::remove_cv_t<std::remove_reference_t<Epi>>;
    using AuxT = decltype(pre(0));
    using PL = Policy<PG, PipeT>;
    Pending<EpiT, AuxT> cur{epi, f32x16{}, AuxT{}, 0};
    static_for<NT>([&](auto t_c) VDN_INL {
        constexpr int T = decltype(t_c)::value;
        constexpr int CC = C + T;
        constexpr int NS = 2 * PG::kt(CC), NG = (NS + kGroup - 1) / kGroup;
        auto aux_cur = pre(T);                                  // loads for this tile's epilogue (runs in step CC + 1)
        f32x16 acc_cur;
        if constexpr (T == 0) {
            // the previous layer's last tile: before the MFMA group that reads it (group 1 at the latest keeps the barrier first)
            constexpr int TP = PendIn::tile;
            constexpr int glimit = (PREV_WRITES_INPUT && TP >= 0) ? (2 * TP) / kGroup : NG;
            if constexpr (glimit == 0) {        // the pending tile is read by this step's very first MFMAs: nothing to hide under
                f.pend.run();
                acc_cur = cstream::chunk_step<PL, CC>(pp, X, [](auto, auto) VDN_INL {}).w;
            } else {
                constexpr int G = glimit > 1 ? 1 : 0;
                acc_cur = cstream::chunk_step<PL, CC>(pp, X, in_group<G>([&]() VDN_INL { f.pend.run(); })).w;
            }
        } else {
            acc_cur = cstream::chunk_step<PL, CC>(pp, X, in_group<1>([&]() VDN_INL { cur.run(); })).w;
        }
        cur.acc = acc_cur;
        cur.aux = aux_cur;
        cur.nt = T;
        __builtin_amdgcn_sched_barrier(0);
    });
    using Out = Pending<EpiT, AuxT, NT - 1>;
    return Flow<C + NT, Out>{Out{cur.epi, cur.acc, cur.aux, cur.nt}};
}

template <int C, class Pend>
VDN_DEV void flow_finish(Flow<C, Pend>& f) { f.pend.run(); }
// run the pending epilogue now (code between two layers needs the previous layer's last tile): no overlap at this boundary
template <int C, class Pend>
VDN_DEV Flow<C, NoPend> flow_drain(Flow<C, Pend>& f) {
    f.pend.run();
    __builtin_amdgcn_sched_barrier(0);
    return Flow<C, NoPend>{NoPend{}};
}
VDN_DEV Flow<0, NoPend> flow_begin() { return Flow<0, NoPend>{NoPend{}}; }

struct NoLoad {
    VDN_DEV int operator()(int) const { return 0; }
};

}  // namespace flow
}  // namespace vdn
