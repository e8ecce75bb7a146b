"""savgol_streambank_push_block at every tile, strip and ring seam, through the C ABI.

tests/stream_seams.py holds the matrix as plain functions (its docstring has the checks and the bars); tests/test_stream_block_forms.py accounts for it on
a CPU -- which form every call takes, that each form of each (half window, bank) is taken, that the shapes meant to have a partial last group have one.
  1. test_block_push_seam_matrix: the case list of every (half window, bank), in-process.
  2. test_forms_behind_the_switches: SAVGOL_HIP_STREAM_DMA=0 (the walk on whole aligned strips, register tiles in whole groups), SAVGOL_HIP_STREAM_MOMENT=0
     (moment-shaped filters on the tap-by-tap tiles) and SAVGOL_HIP_SMALL_SERVICE=0 (sg_stream_rows_kernel's launch path under the single-stream API, and the
     short host-pointer savgol_apply beside it): the library reads the switches once per process, so each runs `python -m tests.stream_seams` in one fresh
     child process.
  3. test_block_push_refuses_overlap: d_out sharing a byte with d_samples is refused before any launch and leaves the bank as it was."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stream_seams as seams
from tests._util import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu(sg):
    import torch
    assert torch.cuda.is_available() and sg.device_count() > 0, sg.last_error()
    return torch


@pytest.mark.parametrize("n,fma", [(n, fma) for n in seams.HALF_WINDOWS for fma in (0, 1)])
def test_block_push_seam_matrix(sg, sgo, torch_gpu, n, fma):
    """Every case of seams.cases(n, fma): fresh bank, tick pushes up to the history the case asks for, the block calls, both flushes, 2n + 1 more ticks.
    Bit-exact bank: 0 differing words on every stream.  Fused bank: under fp32_bar(the restatement's own error) of the double sum over the whole bank.
    Guards around d_out and d_samples intact, d_samples unchanged, return values and counters the oracle's, after every call."""
    stats = seams.run_list(sg, torch_gpu, seams.cases(n, fma), seed=100 * n + fma)
    print(f"n={n} {'fused' if fma else 'bit-exact'} bank: {stats}")
    assert stats.cases and stats.blocks and stats.outputs


@pytest.mark.parametrize("switch", sorted(seams.CHILDREN))
def test_forms_behind_the_switches(torch_gpu, switch):
    env = dict(os.environ)
    env[switch] = "0"
    argv, limit = seams.CHILDREN[switch]                                     # each child under a time limit of its own
    done = subprocess.run([sys.executable, "-m", "tests.stream_seams"] + argv, env=env, cwd=seams.ROOT, timeout=limit,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(done.stdout[-2000:])
    assert done.returncode == 0, (switch, done.returncode, done.stdout[-6000:])


def test_block_push_refuses_overlap(sg, sgo, torch_gpu):
    """[d_samples, d_samples + ticks x streams) and [d_out, d_out + ticks x streams) may not share a byte: -1 with "overlap" in the error text, before any
    launch -- the samples and the guard rows around them stay as they were, the counters too, and the bank then continues its sequence to the oracle's bits
    (so the ring was not touched either).  Buffers that touch end to start are accepted, in either order."""
    torch = torch_gpu
    S, n, T = 256, 8, 64
    ws = 2 * n + 1
    case = seams.Case("overlap", S, 0, 0, n, 4, 0, 1.0, 0, 0.0, ())
    x = seams.signal(case, 3 * T, 5)
    filt = sgo.Filter(n, 4, 0, 1.0)
    ref = seams.dot_rows(filt.center, filt.dt_inv, x, np.float32)
    buf = torch.from_numpy(x).cuda()                                        # rows 0..T | T..2T | 2T..3T
    before = buf.clone()
    bank = sg.StreamBank(S, n, 4, 0, 1.0)
    warm = torch.full((ws + 3, S), -7.0, device="cuda")
    assert bank.push_block(buf, ws + 3, warm) == 4                          # a ready bank with a wrapped ring
    row = S * 4
    for shift in (0, -row, row, -(T * row - 4), T * row - 4):               # the same rows, one row behind / ahead, and a single shared element at either end
        assert bank.push_block(buf.data_ptr() + T * row, T, buf.data_ptr() + T * row + shift) == -1, shift
        assert "overlap" in sg.last_error()
        assert bank.counters == (ws + 3, 4)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # touching end to start: d_out right behind d_samples, then right in front of them
    assert bank.push_block(buf.data_ptr() + (ws + 3) * row, T, buf.data_ptr() + (ws + 3 + T) * row) == T, sg.last_error()
    torch.cuda.synchronize()
    got = buf[ws + 3 + T:ws + 3 + 2 * T].cpu().numpy()
    assert same_bits(got, ref[ws + 3 - 2 * n:ws + 3 - 2 * n + T])
    bank2 = sg.StreamBank(S, n, 4, 0, 1.0)
    buf.copy_(before)
    assert bank2.push_block(buf.data_ptr() + T * row, T, buf.data_ptr()) == T - 2 * n, sg.last_error()
    torch.cuda.synchronize()
    assert same_bits(buf[2 * n:T].cpu().numpy(), seams.dot_rows(filt.center, filt.dt_inv, x[T:2 * T], np.float32))
    assert torch.equal(buf[T:], before[T:])
