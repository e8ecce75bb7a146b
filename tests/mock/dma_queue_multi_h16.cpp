// dma_queue_multi_h16.cpp -- tests/mock/dma_queue_multi.cpp for the fused multi-output stream tiles on 16-bit rows (csrc/sg_stream_dma_multi_st16.hip): a
// DMA moves FOUR rows of 256 bytes and a finished output row issues K stores.  Holds DmaQueue<N, 32, DP, 4, K> (csrc/sg_stream_host.hpp) to a simulation
// of the wave's vector-memory queue: the DP DMAs of the prologue, then per step the K stores of every output row the step's four rows finish (pad rows of
// an odd half window finish none) and the next DMA; at every wait the kernel issues -- the centre wait (the first eight rows = DMA 1), the first wait,
// one per step -- the operations younger than the DMA waited for are counted.  Half windows 1 .. 16, the ring depths multi_h16_tile_shape ships
// (in rows; four rows per DMA; clamped to the tile, as the launcher clamps them) and both depths of the table for every half window.  Prints one line
// per (N, DP, K).  Plain g++.
#include <cstdio>
#include <vector>

#include "sg_stream_host.hpp"

template <int N, int DP, int K>
static int check(bool shipped)
{
    constexpr int TR = 32, RPD = 4;
    typedef sg::DmaQueue<N, TR, DP, RPD, K> Q;
    constexpr int ROWS = TR + 2 * N, NI = (ROWS + RPD - 1) / RPD;
    static_assert(DP >= 2 && DP <= NI, "the kernel's own bounds on the ring");
    if (Q::NI != NI) { printf("N=%d DP=%d K=%d: NI %d, simulated %d\n", N, DP, K, Q::NI, NI); return 1; }
    std::vector<int> queue;                                   // issue order: >= 0 = DMA index, -1 = a store
    auto younger = [&](int p) { int at = -1; for (size_t i = 0; i < queue.size(); ++i) if (queue[i] == p) at = (int)i; return at < 0 ? -1 : (int)queue.size() - 1 - at; };
    for (int i = 0; i < DP; ++i) queue.push_back(i);
    int waits = 0;
    if (younger(1) != Q::younger(1, 0)) { printf("N=%d DP=%d K=%d: centre wait for DMA 1: queue %d, DmaQueue %d\n", N, DP, K, younger(1), Q::younger(1, 0)); return 1; }
    ++waits;
    if (younger(0) != Q::younger(0, 0)) { printf("N=%d DP=%d K=%d: first wait: queue %d, DmaQueue %d\n", N, DP, K, younger(0), Q::younger(0, 0)); return 1; }
    ++waits;
    for (int g = 0; g < NI; ++g) {
        if (g + 1 < NI) {
            const int sim = younger(g + 1);
            if (sim < 0 || sim != Q::younger(g + 1, g)) { printf("N=%d DP=%d K=%d: step %d waits for DMA %d: queue %d, DmaQueue %d\n", N, DP, K, g, g + 1, sim, Q::younger(g + 1, g)); return 1; }
            ++waits;
        }
        for (int r = RPD * g; r < RPD * g + RPD; ++r)
            if (r < ROWS && r >= 2 * N && r - 2 * N < TR)                                // pad rows (r >= ROWS) are never fed
                for (int k = 0; k < K; ++k) queue.push_back(-1);                         // output row r - 2N has seen its last row: one store per output
        if (g + DP < NI) queue.push_back(g + DP);
    }
    int stores = 0, dmas = 0;
    for (int q : queue) { if (q < 0) ++stores; else ++dmas; }
    if (stores != K * TR || dmas != NI) { printf("N=%d DP=%d K=%d: %d stores, %d DMAs\n", N, DP, K, stores, dmas); return 1; }
    printf("N=%d DP=%d K=%d: ok waits=%d%s\n", N, DP, K, waits, shipped ? " shipped" : "");
    return 0;
}

template <int N, int K>
static int depths()
{
    constexpr int NI = (32 + 2 * N + 3) / 4;
    constexpr int fused = sg::multi_h16_tile_shape(N, true, K).rows / 4, exact = sg::multi_h16_tile_shape(N, false, K).rows / 4;
    constexpr int a = 6 < NI ? 6 : NI, b = 8 < NI ? 8 : NI, f = fused < NI ? fused : NI, e = exact < NI ? exact : NI;
    // the two depths 6 and 8 DMAs = 24 and 32 rows (clamped), each marked `shipped` where a launch of the table uses it at this half window
    const bool fs = N <= sg::stream_multi_h16_max_n(true, K), es = N <= sg::stream_multi_h16_max_n(false, K);
    int bad = check<N, a, K>((fs && f == a) || (es && e == a));
    if (b != a) bad += check<N, b, K>((fs && f == b) || (es && e == b));
    if (fs && f != a && f != b) bad += check<N, f, K>(true);
    if (es && e != a && e != b && e != f) bad += check<N, e, K>(true);
    return bad;
}

constexpr int kTop = 16;                                      // past every shipped bound: the rule, not only the table, is pinned
template <int N>
static int every()
{
    int bad = depths<N, 2>() + depths<N, 3>();
    if constexpr (N < kTop) bad += every<N + 1>();
    return bad;
}

int main()
{
    static_assert(sg::stream_multi_h16_max_n(true, 2) <= kTop && sg::stream_multi_h16_max_n(true, 3) <= kTop && sg::stream_multi_h16_max_n(false, 2) <= kTop &&
                  sg::stream_multi_h16_max_n(false, 3) <= kTop, "raise kTop with the bounds");
    const int bad = every<1>();
    printf("bounds fused %d %d exact %d %d\n", sg::stream_multi_h16_max_n(true, 2), sg::stream_multi_h16_max_n(true, 3), sg::stream_multi_h16_max_n(false, 2),
           sg::stream_multi_h16_max_n(false, 3));
    printf("mismatches %d\n", bad);
    return bad ? 1 : 0;
}
