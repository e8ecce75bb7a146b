"""The s_waitcnt vmcnt counts of the LDS-DMA stream tiles, held to a simulated queue on a CPU.

The tiles issue all their row loads as LDS-DMA and consume the rows in arrival order behind counted waits: before step g a wave waits until at most
DmaQueue::younger(g + 1, g) vector-memory operations younger than DMA g + 1 are outstanding (csrc/sg_stream_host.hpp).  A count one too large lets a
step read rows that have not landed -- on the GPU that shows only as occasional wrong bits.  tests/mock/dma_queue.cpp issues what the kernels issue, in
their order (the prologue's DMAs, then per step the stores of the outputs its rows finish and the next DMA), into a plain list and counts the entries
behind the DMA waited for, at every wait the kernels issue: the centre wait of the fused bank's centred tiles, the first wait, and one per step.
Every half window 1..32, tiles of 32 ticks, the ring depths of the launch tables (12 and 16 KiB of fp32 row pairs; 6 and 8 KiB of 16-bit row quads) and
the depths of their A/B alternatives, 2 rows per DMA (the rule the fp32 kernels ship with: it pins the simulator) and 4 (the 16-bit kernels).  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("dma_queue")), "dma_queue")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "dma_queue.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    return done.returncode, done.stdout.splitlines()


def test_every_wait_counts_what_the_queue_holds(report):
    code, lines = report
    bad = [l for l in lines[:-1] if not re.search(r": ok waits=\d+$", l)]
    assert not bad and code == 0 and lines[-1] == "mismatches 0", bad[:5]


def test_the_table_covers_both_row_counts_and_the_launch_tables(report):
    _, lines = report
    seen = set()
    for l in lines[:-1]:
        m = re.match(r"N=(\d+) DP=(\d+) RPD=(\d+): ok waits=(\d+)$", l)
        assert m, l
        n, dp, rpd, waits = map(int, m.groups())
        ni = (32 + 2 * n + rpd - 1) // rpd
        assert dp <= ni and waits == ni + 1                                # the centre wait, the first wait, one per step but the last
        seen.add((n, dp, rpd))
    for n in range(1, 33):
        for depth in (12, 16):                                             # launch_bank_dma_shape / launch_bank_dma_mom, clamped to the tile
            assert (n, min(depth, (32 + 2 * n) // 2), 2) in seen
            assert (n, min(depth // 2, (32 + 2 * n + 3) // 4), 4) in seen
