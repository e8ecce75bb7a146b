"""savgol_streambank_push_block_i16 on a CPU: the symbol and its ctypes binding, the refusal that needs no device, the amplitudes of the GPU test's
signals (tests/test_gpu_stream_i16.py) against their purpose, and the resources of the new kernels from the built code objects: the body tile on
int16 rows (sg_bank_dma_i16_kernel, one instance per instance of the 16-bit float tile) and the three small kernels of the route.  The route a call
takes is block_plan_h16's, which knows only that an element is two bytes: tests/test_stream_h16_host.py holds it to its rule.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import stream_seams as seams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")
NAME = "savgol_streambank_push_block_i16"


def test_symbol_exported_and_bound(sg):
    assert NAME in sg.SIGNATURES
    fn = getattr(sg.lib(), NAME)
    assert len(fn.argtypes) == 6
    assert hasattr(sg.StreamBank, "push_block_i16")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == NAME for line in out.splitlines())
    # nothing of the new objects leaks past the version script
    assert not [line for line in out.splitlines() if "sg_bank_dma_i16" in line]


def test_refusals_that_need_no_device(sg):
    L = sg.lib()
    assert L.savgol_streambank_push_block_i16(None, 4096, 8, 8192, sg.SAVGOL_HIP_I16, None) == -1
    assert NAME in sg.last_error() and "NULL pointer" in sg.last_error()
    # the NULL pointer comes before the output type
    assert L.savgol_streambank_push_block_i16(None, 4096, 8, 8192, sg.SAVGOL_HIP_F16, None) == -1
    assert NAME in sg.last_error() and "NULL pointer" in sg.last_error()


def test_python_wrapper_refuses_other_output_types(sg):
    for out in ("f16", "bf16", "i32", None):
        with pytest.raises(ValueError):
            sg.StreamBank.push_block_i16(None, 4096, 8, 8192, out)


def test_amplitudes_keep_the_expected_words_inside_the_range(sgo):
    """tests/test_gpu_stream_i16.py's amplitude() against its purpose, on the CPU with dot_rows: for every half window, bank filter and the ride at
    RIDE counts, the samples do not clip and at least half (here: three quarters) of the fp32 results lie strictly inside the int16 range"""
    from tests.test_gpu_stream_i16 import HALF_WINDOWS, RIDE, amplitude, quantise
    for n in HALF_WINDOWS:
        for f in seams.bank_filters(n, 1) + seams.bank_filters(n, 0):
            for offset in (0.0, RIDE) if f[1] > 0 else (0.0,):
                case = seams.Case("amp", 16, 0, 0, n, f[0], f[1], f[2], 1, offset, ())
                x = quantise(case, 400, n, amplitude(n, f, offset)).astype(np.float32)
                assert -32768 < x.min() and x.max() < 32767, (n, f, offset, "the samples themselves clip")
                filt = sgo.Filter(n, f[0], f[1], f[2])
                y = np.rint(seams.dot_rows(filt.center, filt.dt_inv, x, np.float32))
                inside = np.mean((y > -32768) & (y < 32767))
                assert inside >= 0.75, (n, f, offset, inside)
                # and large enough to tell one row from the next; the riding streams (a swing of a few hundred counts, whatever the filter) are there
                # for the centring, where every word still has to be the twin's
                assert np.abs(y).max() >= (4 if offset else 50), (n, f, offset, np.abs(y).max(), "the outputs are too small to tell rows apart")


# waves per SIMD a kernel's VGPRs allow on gfx950 (512 registers per lane and SIMD, allocated in blocks of 8, at most 8 waves)
def occupancy(vgpr):
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def resources(substring):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), LIB, substring], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) spill\s+(\d+) lds\s+(\d+)\s+(?:void )?(\S.*)$", line)
        if m:
            rows[m.group(6)] = dict(vgpr=int(m.group(1)), scratch=int(m.group(3)), spill=int(m.group(4)), lds=int(m.group(5)))
    return rows


@pytest.fixture(scope="module")
def tiles():
    """(int16 tiles, their h16 twins): template arguments -> resources, from the built library"""
    if not (os.path.exists(LIB) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("library or llvm-readelf not present")
    i16 = {k.replace("sg_bank_dma_i16_kernel", ""): v for k, v in resources("sg_bank_dma_i16_kernel").items()}
    h16 = {k.replace("sg_bank_dma_h16_kernel", ""): v for k, v in resources("sg_bank_dma_h16_kernel").items()}
    return i16, h16


def test_new_kernels_have_no_private_segment(tiles):
    i16, h16 = tiles
    # one instance per instance of the 16-bit float tile: half windows 1..32 on both banks, and the block-moment form (12..20, one to three moments)
    # (a half window's instance at the table's last (waves, ring) is built beside the one its launcher takes, as for the 16-bit float tile: 112 in all)
    assert set(i16) == set(h16) and len(i16) == 112, (len(i16), len(h16), sorted(set(i16) ^ set(h16))[:4])
    args = [re.match(r"sg::<(\d+), (true|false), 32, \d+, \d+, \d+, (\d+), ", k).groups() for k in i16]
    assert {(int(n), fma) for n, fma, mom in args if mom == "0"} == {(n, fma) for n in range(1, 33) for fma in ("true", "false")}
    assert {(int(n), int(mom)) for n, fma, mom in args if mom != "0"} == {(n, mom) for n in range(12, 21) for mom in (1, 2, 3)}
    for key, r in i16.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (key, r)
        assert r["lds"] == h16[key]["lds"] == 0, (key, r)                    # the rings are dynamic LDS, sized by the launcher
    small = resources("i16")
    for name in ("sg_i16_widen_kernel", "sg_i16_round_kernel", "sg_bank_store_tail_i16_kernel"):
        found = [v for k, v in small.items() if name in k]
        assert len(found) == 1, (name, sorted(small))
        assert found[0]["scratch"] == 0 and found[0]["spill"] == 0 and found[0]["vgpr"] <= 64, (name, found[0])


def test_new_tiles_keep_their_h16_twins_occupancy_step(tiles):
    """every int16 tile's VGPRs at or under its h16 twin's occupancy step.
    The instance this test exists for is the block-moment tile at n = 15 with three moments: 96 VGPRs like its twin, through the int16 build's store
    order and the occupancy hint of its launch bounds; without them it has 98, one step down."""
    i16, h16 = tiles
    over = {key: (r["vgpr"], h16[key]["vgpr"]) for key, r in i16.items() if occupancy(r["vgpr"]) < occupancy(h16[key]["vgpr"])}
    print({key: v for key, v in over.items()})
    assert not over, over
