// dma_queue.cpp -- holds DmaQueue (csrc/sg_stream_host.hpp: the s_waitcnt vmcnt counts of the LDS-DMA stream tiles) to a simulation of the wave's
// vector-memory queue.  The simulation issues what the kernels issue, in their order -- the DP DMAs of the prologue, then per step the stores of the
// outputs the step's rows finish and the next DMA -- and at every wait the kernels issue counts the operations younger than the DMA waited for.
// Prints one line per (N, DP, RPD): "ok" or the first mismatch.  Plain g++.  RPD = rows per DMA: 2 (fp32 rows, sg_stream_dma.hip), 4 (16-bit rows).
#include <cstdio>
#include <vector>

#include "sg_stream_host.hpp"

template <int N, int TR, int DP, int RPD>
static int check()
{
    typedef sg::DmaQueue<N, TR, DP, RPD> Q;
    constexpr int ROWS = TR + 2 * N, NI = (ROWS + RPD - 1) / RPD;
    if (Q::NI != NI) { printf("N=%d DP=%d RPD=%d: NI %d, simulated %d\n", N, DP, RPD, Q::NI, NI); return 1; }
    if (DP > NI) { printf("N=%d DP=%d RPD=%d: skipped (ring deeper than the tile)\n", N, DP, RPD); return 0; }
    std::vector<int> queue;                                   // issue order: >= 0 = DMA index, -1 = a store
    auto younger = [&](int p) { int at = -1; for (size_t i = 0; i < queue.size(); ++i) if (queue[i] == p) at = (int)i; return at < 0 ? -1 : (int)queue.size() - 1 - at; };
    for (int i = 0; i < DP; ++i) queue.push_back(i);
    int waits = 0;
    // the centre of a centred tile: its first eight rows = the first 8 / RPD DMAs, waited for before step 0 (needs them in the ring together)
    if (8 / RPD <= DP && 8 / RPD <= NI) {
        const int p = 8 / RPD - 1;
        if (younger(p) != Q::younger(p, 0)) { printf("N=%d DP=%d RPD=%d: centre wait for DMA %d: queue %d, DmaQueue %d\n", N, DP, RPD, p, younger(p), Q::younger(p, 0)); return 1; }
        ++waits;
    }
    if (younger(0) != Q::younger(0, 0)) { printf("N=%d DP=%d RPD=%d: first wait: queue %d, DmaQueue %d\n", N, DP, RPD, younger(0), Q::younger(0, 0)); return 1; }
    ++waits;
    for (int g = 0; g < NI; ++g) {
        if (g + 1 < NI) {
            const int sim = younger(g + 1);
            if (sim < 0 || sim != Q::younger(g + 1, g)) { printf("N=%d DP=%d RPD=%d: step %d waits for DMA %d: queue %d, DmaQueue %d\n", N, DP, RPD, g, g + 1, sim, Q::younger(g + 1, g)); return 1; }
            ++waits;
        }
        for (int r = RPD * g; r < RPD * g + RPD; ++r)
            if (r < ROWS && r >= 2 * N && r - 2 * N < TR) queue.push_back(-1);      // output r - 2N has seen its last row: one store
        if (g + DP < NI) queue.push_back(g + DP);
    }
    int stores = 0, dmas = 0;
    for (int q : queue) { if (q < 0) ++stores; else ++dmas; }
    if (stores != TR || dmas != NI) { printf("N=%d DP=%d RPD=%d: %d stores, %d DMAs\n", N, DP, RPD, stores, dmas); return 1; }
    printf("N=%d DP=%d RPD=%d: ok waits=%d\n", N, DP, RPD, waits);
    return 0;
}

template <int N, int DP>
static int both()
{
    constexpr int NI2 = (32 + 2 * N) / 2, NI4 = (32 + 2 * N + 3) / 4;
    // the launchers clamp the ring to the tile: DP = min(table depth, NI); the 16-bit tables hold half the fp32 depth
    return check<N, 32, (DP < NI2 ? DP : NI2), 2>() + check<N, 32, (DP / 2 < NI4 ? DP / 2 : NI4), 4>() + check<N, 32, (DP < NI4 ? DP : NI4), 4>();
}

template <int N>
static int every()
{
    int bad = both<N, 8>() + both<N, 12>() + both<N, 16>() + both<N, 24>();      // 12, 16: the launch tables; 8, 24: the A/B alternatives
    if constexpr (N < 32) bad += every<N + 1>();
    return bad;
}

int main()
{
    const int bad = every<1>();
    printf("mismatches %d\n", bad);
    return bad ? 1 : 0;
}
