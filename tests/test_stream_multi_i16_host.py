"""savgol_streambank_push_block_multi_i16 on a CPU: both symbols and their ctypes bindings, the refusals that need no device and their order, the route
every call takes, the resources of the new kernels from the built code objects, and the amplitudes of the GPU test's signals against their purpose.

csrc/sg_stream_host.hpp (block_plan_multi_i16) is built with plain g++ into tests/mock/stream_block_multi_i16.cpp, which prints one line per call shape;
every line is held to the rule restated here from the call's contract (include/savgol_hip.h, csrc/sg_stream_host.hpp) -- block_plan_multi_h16's, with the
int16 call's own bound and shape tables:
  FUSED   count >= 2; every bank the same half window n and the same SAVGOL_STREAMBANK_FMA flag; n <= MAX_N[bank kind, outputs per launch]; streams %
          128 == 0, rows under the descriptor limit, the int16 sample base, every output base and every ring 16-byte aligned (`mis` = their low four
          bits, or-ed), more than 64 ticks; every bank's twin takes tap-by-tap LDS-DMA tiles (block_form, restated as in tests/test_stream_h16_host.py:
          not the block moments, both switches on); tile counts 32 bits index.  2 or 3 outputs are one launch, 4 are two launches of two.  head = 64,
          body = ticks - 64, and the body's tiles are tile_geom(streams, 128, body, 32, 128 strips per group, the launch table's waves per block: 4 waves
          and a ring of 32 rows, but 8 and 24 for the fused bank at n = 6 with two outputs per launch).
  SINGLE  everything else: `count` single savgol_streambank_push_block_i16 calls.
No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import stream_multi_i16 as mi
from tests import stream_seams as seams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")
LIB = os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")
NAME = "savgol_streambank_push_block_multi_i16"
# the shipped bounds: (fused bank?, outputs per launch) -> the largest fused half window
MAX_N = {(0, 2): 8, (0, 3): 8, (1, 2): 8, (1, 3): 8}
F32, F16, BF16, I16 = 0, 1, 2, 3


def test_symbols_exported_and_bound(sg):
    for name, args in ((NAME, 8), (NAME + "_route", 6)):
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == args
    assert callable(sg.push_block_multi_i16) and callable(sg.push_block_multi_i16_route)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    assert NAME in names and NAME + "_route" in names
    # nothing of the new objects leaks past the version script
    assert not [line for line in out.splitlines() if "sg_bank_dma_multi_i16" in line]
    header = open(os.path.join(ROOT, "include", "savgol_hip.h")).read()
    assert NAME + "(" in header and NAME + "_route(" in header
    assert (sg.SAVGOL_HIP_F32, sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16, sg.SAVGOL_HIP_I16) == (F32, F16, BF16, I16)


def test_refusals_that_need_no_device_in_their_order(sg):
    """checks 1 to 5 of the header's order come before anything touches a bank or a device (a bank listed twice is a comparison of two pointers).  Every
    case below carries the fault it is named for AND the next one of the order: the earlier one must be named"""
    L = sg.lib()
    one, two = (C.c_void_p * 1)(4096), (C.c_void_p * 2)(4096, 8192)
    nul, twice = (C.c_void_p * 2)(4096, None), (C.c_void_p * 2)(4096, 4096)
    for fn, tail in ((L.savgol_streambank_push_block_multi_i16, (None, None)), (L.savgol_streambank_push_block_multi_i16_route, ())):
        who = NAME if tail else NAME + "_route"

        def refused(text, banks, count, samples, ticks, outs, out_type):
            assert fn(banks, count, samples, ticks, outs, out_type, *tail) == -1, text
            err = sg.last_error()
            assert err.startswith(who + ":") and text in err, (text, err)

        # 1. NULL banks / d_outs / d_samples (and a count outside 1..4)
        refused("NULL pointer", None, 0, 4096, 8, one, I16)
        refused("NULL pointer", one, 0, None, 8, one, I16)
        refused("NULL pointer", one, 0, 4096, 8, None, I16)
        # 2. count outside 1..4 (and a NULL banks[1])
        for count in (0, -1, 5):
            refused("outside 1..4", nul, count, 4096, 8, two, I16)
        # 3. a NULL banks[k] or d_outs[k] (and an unserved output type)
        refused("NULL pointer: banks[1]", nul, 2, 4096, 8, two, BF16)
        refused("NULL pointer: d_outs[1]", two, 2, 4096, 8, nul, BF16)
        # 4. an unserved output type, named (and a bank listed twice)
        for ot, text in ((F16, "output type f16 (1)"), (BF16, "output type bf16 (2)"), (7, "output type unknown (7)"), (-1, "output type unknown (-1)")):
            refused(text, twice, 2, 4096, 8, two, ot)
        # 5. a bank listed twice (decided before a bank is looked into: these are no banks)
        refused("listed twice", twice, 2, 4096, 8, two, I16)
        refused("listed twice", twice, 2, 4096, 8, two, F32)


def test_python_wrapper_refuses_other_output_types(sg):
    for out in ("f16", "bf16", "i32", None):
        with pytest.raises(ValueError):
            sg.push_block_multi_i16([1, 2], 4096, 8, [4096, 8192], out)
        with pytest.raises(ValueError):
            sg.push_block_multi_i16_route([1, 2], 4096, 8, [4096, 8192], out)
    with pytest.raises(ValueError):
        sg.push_block_multi_i16([1, 2], 4096, 8, [4096])


FILTERS = ((0, 0), (0, 2), (1, 2), (1, 3))                                 # (centre, moment terms): smoothing; one the fit takes; centred linear; centred quadratic


def shapes():
    """(count, streams, ticks, misaligned, dma_switch, moment_switch, ((n, fma, centre, terms), ...))"""
    out = []

    def banks(count, n, fma, first=0):
        return tuple((n, fma, FILTERS[(first + k) % 4][0] if fma else 0, FILTERS[(first + k) % 4][1]) for k in range(count))

    for n in (1, 5, 6, 8, 9, 12, 16, 17, 32):
        for fma in (0, 1):
            for count in (1, 2, 3, 4):
                for streams in (1, 127, 128, 129, 130, 256, 2176, 16512):
                    for ticks in (1, 63, 64, 65, 96, 97, 4096):
                        out.append((count, streams, ticks, 0, 1, 1, banks(count, n, fma, len(out))))
                # one base off the 16-byte grid -- the samples, an output or a ring, 2, 4 or 8 bytes: the or of the low four bits is what the rule sees
                for mis in (2, 4, 8):
                    for ticks in (65, 97):
                        out.append((count, 256, ticks, mis, 1, 1, banks(count, n, fma)))
                for dma, mom in ((0, 1), (1, 0), (0, 0)):                  # SAVGOL_HIP_STREAM_DMA=0 / SAVGOL_HIP_STREAM_MOMENT=0
                    out.append((count, 256, 97, 0, dma, mom, banks(count, n, fma)))
                    out.append((count, 2176, 4096, 0, dma, mom, banks(count, n, fma, 1)))
        # mixed flags and mixed half windows in one call
        for count in (2, 3, 4):
            mixed = tuple((n, k & 1, 0, 0) for k in range(count))
            out.append((count, 256, 97, 0, 1, 1, mixed))
            other = 5 if n != 5 else 6
            out.append((count, 256, 97, 0, 1, 1, tuple((other if k == count - 1 else n, 1, 0, 0) for k in range(count))))
            out.append((count, 2176, 4096, 0, 1, 1, tuple((other if k == 0 else n, 0, 0, 0) for k in range(count))))
    # config 3's shape, rows at the descriptor limit, and a tile count 32 bits do not index
    out += [(3, 65536, 4096, 0, 1, 1, ((4, 1, 0, 0), (4, 1, 1, 2), (4, 1, 1, 3))), (2, 65536, 4096, 0, 1, 1, ((8, 0, 0, 0), (8, 0, 0, 0))),
            (2, 0x7fffff00 // 4, 97, 0, 1, 1, ((4, 1, 0, 0), (4, 1, 0, 0))), (2, 0x7fffff00 // 4 - 128, 97, 0, 1, 1, ((4, 1, 0, 0), (4, 1, 0, 0))),
            (2, 1 << 27, 1 << 20, 0, 1, 1, ((4, 0, 0, 0), (4, 0, 0, 0)))]
    return out


def tile_geom(streams, strip_width, ticks, tr, group, wpb):
    strips = -(-streams // strip_width)
    bands = -(-ticks // tr)
    group = min(group, strips)
    total = -(-strips // group) * group * bands
    grid = 0 if total >= 0x7fffff00 else (-(-total // wpb) + 7) & ~7
    return strips, bands, group, total, grid


def twin_form(n, fma, streams, ticks, mis, centre, terms, dma, mom):
    """block_form, as tests/test_stream_h16_host.py restates it: the family of the twin's tiles"""
    if dma and streams % 128 == 0 and streams * 4 < 0x7fffff00 and mis == 0 and ticks >= 64:
        if fma and mom and 12 <= n <= 20 and terms > 0 and not (centre and terms >= 3):
            return "MOMENT_TILES"
        if n <= 16 or fma or n >= 20:
            return "DMA_TILES"
    return "OTHER"


def rule(count, streams, ticks, mis, dma, mom, banks):
    head = (f"count={count} streams={streams} ticks={ticks} mis={mis} dma={dma} mom={mom} banks=" + ",".join("/".join(str(v) for v in b) for b in banks) + ":")
    per = (2, 2) if count == 4 else (count, 0)
    n, fma = banks[0][0], banks[0][1]
    fused = (count >= 2 and all(b[0] == n and b[1] == fma for b in banks) and n <= MAX_N[(fma, per[0])] and ticks > 64 and
             all(twin_form(n, fma, streams, ticks, mis, b[2], b[3], dma, mom) == "DMA_TILES" for b in banks))
    if fused:
        twin_wpb = 8 if 5 < n <= 11 and fma else 4                          # launch_bank_dma_i16_shape's
        wpb, rows = (8, 24) if (n, fma, per[0]) == (6, 1, 2) else (4, 32)   # multi_i16_tile_shape's
        geo = tile_geom(streams, 128, ticks - 64, 32, 128, wpb)
        if tile_geom(streams, 128, ticks, 32, 128, twin_wpb)[4] == 0 or geo[4] == 0:
            fused = False
    if not fused:
        return f"{head} SINGLE calls={count}"
    return (f"{head} FUSED launches={2 if count == 4 else 1} per={per[0]},{per[1]} head=64 body={ticks - 64} wpb={wpb} rows={rows} "
            "strips=%d bands=%d group=%d total=%d grid=%d" % geo)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("stream_block_multi_i16")), "stream_block_multi_i16")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "stream_block_multi_i16.cpp")],
                   check=True)
    text = "".join(" ".join(str(v) for v in shape[:6]) + " " + " ".join(" ".join(str(v) for v in b) for b in shape[6]) + "\n" for shape in shapes())
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def test_the_bounds_are_the_ones_restated_here(lines):
    assert lines[-1] == "bounds fused %d %d exact %d %d" % (MAX_N[(1, 2)], MAX_N[(1, 3)], MAX_N[(0, 2)], MAX_N[(0, 3)])
    assert mi.FUSED_MAX_N == MAX_N                                         # the GPU test restates the same table


def test_every_plan_follows_the_rule(lines):
    want = [rule(*shape) for shape in shapes()]
    got_all = lines[:-1]
    assert len(got_all) == len(want)
    bad = [(got, exp) for got, exp in zip(got_all, want) if got != exp]
    for got, exp in bad[:8]:
        print(f"rule: {exp}\nplan: {got}")
    assert not bad, f"{len(bad)} of {len(want)} plans differ from the rule"


def test_the_table_takes_both_routes(lines):
    lines = lines[:-1]
    text = "\n".join(lines)
    for word in ("FUSED launches=1 per=2,0", "FUSED launches=1 per=3,0", "FUSED launches=2 per=2,2", "SINGLE calls=1", "SINGLE calls=4", "wpb=8 rows=24", "wpb=4 rows=32"):
        assert word in text, word
    assert sum(" FUSED " in l for l in lines) >= 100
    for l in lines:
        f = dict(kv.split("=") for kv in l.split(":")[0].split())
        banks = [tuple(int(v) for v in b.split("/")) for b in f["banks"].split(",")]
        if (f["count"] == "1" or f["mis"] != "0" or int(f["streams"]) % 128 or int(f["ticks"]) <= 64 or f["dma"] == "0" or len({b[:2] for b in banks}) > 1 or
                banks[0][0] > max(MAX_N.values())):
            assert l.endswith(f" SINGLE calls={f['count']}"), l
    # the bounds of the table: n = 8 | 9, ticks 64 | 65, streams 128 | 129 | 2176, on both bank kinds and for two outputs
    for fma in (0, 1):
        def route(n, streams, ticks):
            (l,) = [l for l in lines if l.startswith(f"count=2 streams={streams} ticks={ticks} mis=0 dma=1 mom=1 banks={n}/{fma}/")]
            return " FUSED " in l
        assert route(8, 128, 65) == (MAX_N[(fma, 2)] >= 8) and not route(9, 128, 65)
        assert not route(5, 128, 64) and route(5, 128, 65) and not route(5, 129, 65) and route(5, 2176, 65)
    # the block moments are no reason to leave: fused half windows lie below their range, whatever the fit says
    assert any(" FUSED " in l and "/1/1/3" in l for l in lines)
    # config 3's shape, three outputs: 512 strips x 126 bands of the body in 16 128 blocks of four waves
    assert any(l.startswith("count=3 streams=65536 ticks=4096 ") and l.endswith("head=64 body=4032 wpb=4 rows=32 strips=512 bands=126 group=128 total=64512 grid=16128") for l in lines)


# ---- resources of the new kernels, from the built code objects (as tests/test_stream_i16_host.py reads them) ----
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
    """(int16 fused tiles, their h16 twins): template arguments -> resources, from the built library"""
    if not (os.path.exists(LIB) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("library or llvm-readelf not present")
    i16 = {k.replace("sg_bank_dma_multi_i16_kernel", ""): v for k, v in resources("sg_bank_dma_multi_i16_kernel").items()}
    h16 = {k.replace("sg_bank_dma_multi_h16_kernel", ""): v for k, v in resources("sg_bank_dma_multi_h16_kernel").items()}
    return i16, h16


def test_new_kernels_have_no_private_segment(tiles):
    i16, h16 = tiles
    # one instance per (half window up to the bound, bank kind, two or three outputs), at the shape table's (waves per block, ring)
    args = [re.match(r"sg::<(\d+), (true|false), (\d), 32, (\d+), (\d+), \d+>", k).groups() for k in i16]
    assert len(args) == len(i16) > 0
    want = {(n, fma, k) for fma in (0, 1) for k in (2, 3) for n in range(1, MAX_N[(fma, k)] + 1)}
    assert {(int(n), int(fma == "true"), int(k)) for n, fma, k, _, _ in args} == want and len(i16) == len(want)
    for n, fma, k, wpb, dp in args:
        shape = (8, 24) if (int(n), fma, int(k)) == (6, "true", 2) else (4, 32)
        assert (int(wpb), 4 * int(dp)) == shape, (n, fma, k, wpb, dp)
    for key, r in i16.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (key, r)
        assert r["lds"] == 0, (key, r)                                      # the rings are dynamic LDS, sized by the launcher


def test_new_tiles_keep_their_h16_twins_occupancy_step(tiles):
    """every fused int16 tile's VGPRs at or under the occupancy step of the fused 16-bit float tile at the same (N, FMA, K, shape): the int16 narrow
    needs two temporaries per pair where the bf16 convert needs one, which is where a tile could lose a step"""
    i16, h16 = tiles
    assert set(i16) <= set(h16), sorted(set(i16) - set(h16))[:4]
    for key in sorted(i16):
        print(key, i16[key]["vgpr"], h16[key]["vgpr"])
    over = {key: (r["vgpr"], h16[key]["vgpr"]) for key, r in i16.items() if occupancy(r["vgpr"]) < occupancy(h16[key]["vgpr"])}
    assert not over, over


# ---- the amplitudes of the GPU test's signals: a condition, not a measurement ----
def test_amplitudes_keep_the_expected_words_inside_the_range(sgo):
    """for every (half window, filter) tests/test_gpu_stream_multi_i16.py uses -- plain and riding at RIDE counts --, the expected int16 words from the
    oracle's taps in the reference's order (stream_seams.dot_rows), converted as the contract says: the samples do not clip, at least half of the words
    lie strictly inside (-32768, 32767) and the largest magnitude is at least MIN_PEAK = 10 counts"""
    assert set(mi.HALF_WINDOWS) >= {4, 8, 9}
    for n in mi.HALF_WINDOWS:
        for offset in (0.0, mi.RIDE):
            x = mi.quantise(256, n, 400, n, offset).astype(np.float32)
            assert -32768 < x.min() and x.max() < 32767, (n, offset, "the samples themselves clip")
            for f in mi.filters_for(n, sgo):
                filt = sgo.Filter(n, f[0], f[1], f[2])
                y = seams.dot_rows(filt.center, filt.dt_inv, x, np.float32)
                words = np.clip(np.rint(np.nan_to_num(y, nan=0.0)), -32768, 32767).astype(np.int16)
                assert mi.inside_enough(words), (n, f, offset, "fewer than half of the expected words are inside the int16 range")
                assert int(np.abs(words.astype(np.int64)).max()) >= mi.MIN_PEAK, (n, f, offset, int(np.abs(words.astype(np.int64)).max()))
