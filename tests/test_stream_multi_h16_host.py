"""savgol_streambank_push_block_multi_h16 on a CPU: both symbols and their ctypes bindings, the refusals that need no device and their order, and the
route every call takes.

csrc/sg_stream_host.hpp (block_plan_multi_h16) is built with plain g++ into tests/mock/stream_block_multi_h16.cpp, which prints one line per call shape;
every line is held to the rule restated here from the call's contract (include/savgol_hip.h, csrc/sg_stream_host.hpp) -- the conjunction of what the
fp32 fused call (block_plan_multi) and the single 16-bit call's tile route (block_plan_h16) demand:
  FUSED   count >= 2; every bank the same half window n and the same SAVGOL_STREAMBANK_FMA flag; n <= MAX_N[bank kind, outputs per launch]; streams %
          128 == 0, rows under the descriptor limit, the 16-bit sample base, every output base and every ring 16-byte aligned (`mis` = their low four
          bits, or-ed), more than 64 ticks; every bank's twin takes tap-by-tap LDS-DMA tiles (block_form, restated as in tests/test_stream_h16_host.py:
          not the block moments, both switches on); tile counts 32 bits index.  2 or 3 outputs are one launch, 4 are two launches of two.  head = 64,
          body = ticks - 64, and the body's tiles are tile_geom(streams, 128, body, 32, 128 strips per group, the launch table's waves per block: 4 waves
          and a ring of 32 rows, but 8 and 24 for the fused bank at n = 6 with two outputs per launch).
  SINGLE  everything else: `count` single savgol_streambank_push_block_h16 calls.
No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")
NAME = "savgol_streambank_push_block_multi_h16"
# the shipped bounds: (fused bank?, outputs per launch) -> the largest fused half window
MAX_N = {(0, 2): 8, (0, 3): 8, (1, 2): 8, (1, 3): 8}
F32, F16, BF16 = 0, 1, 2


def test_symbols_exported_and_bound(sg):
    for name, args in ((NAME, 9), (NAME + "_route", 7)):
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == args
    assert callable(sg.push_block_multi_h16) and callable(sg.push_block_multi_h16_route)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    assert NAME in names and NAME + "_route" in names
    # nothing of the new objects leaks past the version script
    assert not [line for line in out.splitlines() if "sg_bank_dma_multi_h16" in line]
    header = open(os.path.join(ROOT, "include", "savgol_hip.h")).read()
    assert NAME + "(" in header and NAME + "_route(" in header


def test_refusals_that_need_no_device_in_their_order(sg):
    """checks 1 to 5 of the header's order come before anything touches a bank or a device (a bank listed twice is a comparison of two pointers).  Every
    case below carries the fault it is named for AND the next one of the order: the earlier one must be named"""
    L = sg.lib()
    one, two = (C.c_void_p * 1)(4096), (C.c_void_p * 2)(4096, 8192)
    nul, twice = (C.c_void_p * 2)(4096, None), (C.c_void_p * 2)(4096, 4096)
    for fn, tail in ((L.savgol_streambank_push_block_multi_h16, (None, None)), (L.savgol_streambank_push_block_multi_h16_route, ())):
        who = NAME if tail else NAME + "_route"

        def refused(text, banks, count, samples, in_type, ticks, outs, out_type):
            assert fn(banks, count, samples, in_type, ticks, outs, out_type, *tail) == -1, text
            err = sg.last_error()
            assert err.startswith(who + ":") and text in err, (text, err)

        # 1. NULL banks / d_outs / d_samples (and a count outside 1..4)
        refused("NULL pointer", None, 0, 4096, BF16, 8, one, BF16)
        refused("NULL pointer", one, 0, None, BF16, 8, one, BF16)
        refused("NULL pointer", one, 0, 4096, BF16, 8, None, BF16)
        # 2. count outside 1..4 (and a NULL banks[1])
        for count in (0, -1, 5):
            refused("outside 1..4", nul, count, 4096, BF16, 8, two, BF16)
        # 3. a NULL banks[k] or d_outs[k] (and an unserved pair)
        refused("NULL pointer: banks[1]", nul, 2, 4096, F32, 8, two, BF16)
        refused("NULL pointer: d_outs[1]", two, 2, 4096, F32, 8, nul, BF16)
        # 4. an unserved type pair, named (and a bank listed twice)
        for it, ot, text in ((F32, F32, "f32 -> f32"), (F16, BF16, "f16 -> bf16"), (BF16, F16, "bf16 -> f16"), (F32, F16, "f32 -> f16"), (7, F16, "unknown -> f16")):
            refused(text, twice, 2, 4096, it, 8, two, ot)
        # 5. a bank listed twice (decided before a bank is looked into: these are no banks)
        refused("listed twice", twice, 2, 4096, BF16, 8, two, BF16)
    with pytest.raises(ValueError):
        sg.push_block_multi_h16([1, 2], 4096, "bf16", 8, [4096])
    with pytest.raises(ValueError):
        sg.push_block_multi_h16([1], 4096, "f64", 8, [4096])


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
        twin_wpb = 8 if 5 < n <= 11 and fma else 4                          # launch_bank_dma_h16_shape's
        wpb, rows = (8, 24) if (n, fma, per[0]) == (6, 1, 2) else (4, 32)   # multi_h16_tile_shape's, as measured
        geo = tile_geom(streams, 128, ticks - 64, 32, 128, wpb)
        if tile_geom(streams, 128, ticks, 32, 128, twin_wpb)[4] == 0 or geo[4] == 0:
            fused = False
    if not fused:
        return f"{head} SINGLE calls={count}"
    return (f"{head} FUSED launches={2 if count == 4 else 1} per={per[0]},{per[1]} head=64 body={ticks - 64} wpb={wpb} rows={rows} "
            "strips=%d bands=%d group=%d total=%d grid=%d" % geo)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("stream_block_multi_h16")), "stream_block_multi_h16")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "stream_block_multi_h16.cpp")],
                   check=True)
    text = "".join(" ".join(str(v) for v in shape[:6]) + " " + " ".join(" ".join(str(v) for v in b) for b in shape[6]) + "\n" for shape in shapes())
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def test_the_bounds_are_the_ones_restated_here(lines):
    assert lines[-1] == "bounds fused %d %d exact %d %d" % (MAX_N[(1, 2)], MAX_N[(1, 3)], MAX_N[(0, 2)], MAX_N[(0, 3)])


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
