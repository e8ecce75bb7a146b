"""The s_waitcnt vmcnt counts of the fused multi-output stream tiles (csrc/sg_stream_dma_multi.hip), held to a simulated queue on a CPU.

The multi-output tile is the fp32 LDS-DMA tile with K accumulator sets: a finished output row issues K stores where the single-output tile issues one,
so every count behind a store moves.  DmaQueue (csrc/sg_stream_host.hpp) takes the stores per finished row as a defaulted template parameter; this test
holds DmaQueue<N, 32, DP, 2, K> to tests/mock/dma_queue_multi.cpp, which issues what the kernel issues in its order into a plain list and counts the
entries behind the DMA waited for at every wait the kernel issues: the centre wait (DMA 3: the first eight rows), the first wait, and one per step.
A count one too large lets a step read rows that have not landed -- on the GPU that shows only as occasional wrong bits.
K = 2 and 3; half windows 1 .. 16 (every shipped bound and past it); ring depths 12 and 16 row pairs, clamped to the tile -- the launch table's
(multi_tile_shape) are marked `shipped`.  tests/test_stream_dma_queue.py keeps holding the one-store rule the existing kernels ship with.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("dma_queue_multi")), "dma_queue_multi")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "dma_queue_multi.cpp")], check=True)
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
        ni = (32 + 2 * n) // 2
        assert 4 <= dp <= ni and waits == ni + 1                           # the centre wait, the first wait, one per step but the last
        seen.add((n, dp, k))
        if m.group(5):
            shipped.add((n, dp, k))
    # the launch table, restated from csrc/sg_stream_host.hpp: the fused bank above n = 5 keeps a ring of 12 row pairs, every other tile 16
    for (fma, k), top in bound.items():
        assert 5 <= top <= 16
        for n in range(1, top + 1):
            depth = 12 if fma and n > 5 else 16
            assert (n, min(depth, (32 + 2 * n) // 2), k) in shipped, (fma, k, n)
    for n in range(1, 17):
        for k in (2, 3):
            for depth in (12, 16):
                assert (n, min(depth, (32 + 2 * n) // 2), k) in seen
