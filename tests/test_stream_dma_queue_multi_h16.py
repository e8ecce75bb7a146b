"""The s_waitcnt vmcnt counts of the fused multi-output stream tiles on 16-bit rows (csrc/sg_stream_dma_multi_st16.hip), held to a simulated queue on a CPU.

The kernel combines the 16-bit tile's four rows per DMA with the multi-output tile's K stores per finished output row: DmaQueue<N, 32, DP, 4, K>
(csrc/sg_stream_host.hpp), a combination of template parameters no other kernel instantiates.  tests/mock/dma_queue_multi_h16.cpp issues what the kernel
issues in its order into a plain list and counts the entries behind the DMA waited for at every wait the kernel issues: the centre wait (DMA 1: the first
eight rows), the first wait, and one per step.  A count one too large lets a step read rows that have not landed -- on the GPU that shows only as
occasional wrong bits.  K = 2 and 3; half windows 1 .. 16 (every shipped bound and past it; odd ones have two pad rows that finish no output); ring
depths 24 and 32 rows = 6 and 8 DMAs, clamped to the tile -- the launch table's (multi_h16_tile_shape) are marked `shipped`.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("dma_queue_multi_h16")), "dma_queue_multi_h16")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "dma_queue_multi_h16.cpp")],
                   check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    return done.returncode, done.stdout.splitlines()


def test_every_wait_counts_what_the_queue_holds(report):
    code, lines = report
    bad = [l for l in lines[:-2] if not re.search(r": ok waits=\d+( shipped)?$", l)]
    assert not bad and code == 0 and lines[-1] == "mismatches 0", bad[:5]


def test_the_table_covers_the_shipped_bounds_and_the_launch_table(report):
    _, lines = report
    m = re.match(r"bounds fused (\d+) (\d+) exact (\d+) (\d+)$", lines[-2])
    assert m, lines[-2]
    bound = {(1, 2): int(m.group(1)), (1, 3): int(m.group(2)), (0, 2): int(m.group(3)), (0, 3): int(m.group(4))}
    seen, shipped = set(), set()
    for l in lines[:-2]:
        m = re.match(r"N=(\d+) DP=(\d+) K=(\d+): ok waits=(\d+)( shipped)?$", l)
        assert m, l
        n, dp, k, waits = map(int, m.groups()[:4])
        ni = (32 + 2 * n + 3) // 4                                         # whole DMAs: odd half windows carry two pad rows
        assert 2 <= dp <= ni and waits == ni + 1                           # the centre wait, the first wait, one per step but the last
        seen.add((n, dp, k))
        if m.group(5):
            shipped.add((n, dp, k))
    # the launch table, restated from csrc/sg_stream_host.hpp: a ring of 32 rows (8 DMAs), but 24 rows (6 DMAs) for the fused bank at n = 6 with two outputs
    assert max(bound.values()) >= 1, "no fused shape is shipped"
    for (fma, k), top in bound.items():
        assert 0 <= top <= 8
        for n in range(1, top + 1):
            depth = 6 if (fma, n, k) == (1, 6, 2) else 8
            assert (n, min(depth, (32 + 2 * n + 3) // 4), k) in shipped, (fma, k, n)
    for n in range(1, 17):
        for k in (2, 3):
            for depth in (6, 8):
                assert (n, min(depth, (32 + 2 * n + 3) // 4), k) in seen
