"""savgol_streambank_push_block_multi on a CPU: both symbols and their ctypes bindings, the refusals that need no device, and the route every call takes.

csrc/sg_stream_host.hpp (block_plan_multi) is built with plain g++ into tests/mock/stream_block_multi.cpp, which prints one line per call shape; every
line is held to the rule restated here from the call's contract (include/savgol_hip.h, csrc/sg_stream_host.hpp):
  FUSED   count >= 2; every bank the same half window n and the same SAVGOL_STREAMBANK_FMA flag; n <= MAX_N[bank kind, outputs per launch]; streams %
          128 == 0, rows under the descriptor limit, every pointer 16-byte aligned, more than 64 ticks; every bank's own block push takes tap-by-tap
          LDS-DMA tiles (block_form, restated as in tests/test_stream_h16_host.py: not the block moments, both switches on); tile counts 32 bits index.
          2 or 3 outputs are one launch, 4 are two launches of two.  head = 64, body = ticks - 64, and the body's tiles are tile_geom(streams, 128, body,
          32, 128 strips per group, the launch table's waves per block).
  SINGLE  everything else: `count` single block pushes.
No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")
NAME = "savgol_streambank_push_block_multi"
# the shipped bounds: (fused bank?, outputs per launch) -> the largest fused half window
MAX_N = {(0, 2): 8, (0, 3): 8, (1, 2): 8, (1, 3): 8}


def test_symbols_exported_and_bound(sg):
    for name, args in ((NAME, 7), (NAME + "_route", 5)):
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == args
    assert callable(sg.push_block_multi) and callable(sg.push_block_multi_route)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    assert NAME in names and NAME + "_route" in names
    # nothing of the new objects leaks past the version script
    assert not [line for line in out.splitlines() if "sg_bank_dma_multi" in line]
    header = open(os.path.join(ROOT, "include", "savgol_hip.h")).read()
    assert "#define SAVGOL_STREAM_MULTI_MAX_BANKS 4" in header


def test_refusals_that_need_no_device(sg):
    """checks 1 to 3 of the header's order: they come before anything touches a bank or a device"""
    L = sg.lib()
    one = (C.c_void_p * 1)(4096)
    nul = (C.c_void_p * 1)(None)
    for fn, tail in ((L.savgol_streambank_push_block_multi, (None, None)), (L.savgol_streambank_push_block_multi_route, ())):
        who = NAME if tail else NAME + "_route"

        def refused(text, *args):
            assert fn(*args, *tail) == -1, text
            err = sg.last_error()
            assert err.startswith(who + ":") and text in err, (text, err)

        refused("NULL pointer", None, 1, 4096, 8, one)
        refused("NULL pointer", one, 1, None, 8, one)
        refused("NULL pointer", one, 1, 4096, 8, None)
        for count in (0, -1, 5):
            refused("outside 1..4", one, count, 4096, 8, one)
        refused("NULL pointer: banks[0]", nul, 1, 4096, 8, one)
    with pytest.raises(ValueError):
        sg.push_block_multi([1, 2], 4096, 8, [4096])


FILTERS = ((0, 0), (0, 2), (1, 2), (1, 3))                                 # (centre, moment terms): smoothing; one the fit takes; centred linear; centred quadratic


def shapes():
    """(count, streams, ticks, misaligned, dma_switch, moment_switch, ((n, fma, centre, terms), ...))"""
    out = []

    def banks(count, n, fma, first=0):
        return tuple((n, fma, FILTERS[(first + k) % 4][0] if fma else 0, FILTERS[(first + k) % 4][1]) for k in range(count))

    for n in (1, 5, 6, 8, 9, 12, 16, 17, 32):
        for fma in (0, 1):
            for count in (1, 2, 3, 4):
                for streams in (1, 127, 128, 130, 256, 2176, 16512):
                    for ticks in (1, 63, 64, 65, 96, 97, 4096):
                        out.append((count, streams, ticks, 0, 1, 1, banks(count, n, fma, len(out))))
                for mis in (4, 8):                                         # either pointer 4 or 8 bytes off the 16-byte grid: the or of the low four bits
                    for ticks in (65, 97):
                        out.append((count, 256, ticks, mis, 1, 1, banks(count, n, fma)))
                for dma, mom in ((0, 1), (1, 0), (0, 0)):
                    out.append((count, 256, 97, 0, dma, mom, banks(count, n, fma)))
                    out.append((count, 2176, 4096, 0, dma, mom, banks(count, n, fma, 1)))
        # mixed kinds and mixed half windows in one call
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
    """block_form, as tests/test_stream_h16_host.py restates it: the family of the single block push"""
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
        twin_wpb = 8 if 5 < n <= 11 and fma else 4                          # launch_bank_dma_shape's
        wpb, dp = (8, 12) if n > 5 and fma else (4, 16)                     # multi_tile_shape's
        geo = tile_geom(streams, 128, ticks - 64, 32, 128, wpb)
        if tile_geom(streams, 128, ticks, 32, 128, twin_wpb)[4] == 0 or geo[4] == 0:
            fused = False
    if not fused:
        return f"{head} SINGLE calls={count}"
    return (f"{head} FUSED launches={2 if count == 4 else 1} per={per[0]},{per[1]} head=64 body={ticks - 64} wpb={wpb} dp={dp} "
            "strips=%d bands=%d group=%d total=%d grid=%d" % geo)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("stream_block_multi")), "stream_block_multi")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "stream_block_multi.cpp")],
                   check=True)
    text = "".join(" ".join(str(v) for v in shape[:6]) + " " + " ".join(" ".join(str(v) for v in b) for b in shape[6]) + "\n" for shape in shapes())
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def test_every_plan_follows_the_rule(lines):
    want = [rule(*shape) for shape in shapes()]
    assert len(lines) == len(want)
    bad = [(got, exp) for got, exp in zip(lines, want) if got != exp]
    for got, exp in bad[:8]:
        print(f"rule: {exp}\nplan: {got}")
    assert not bad, f"{len(bad)} of {len(want)} plans differ from the rule"


def test_the_table_takes_both_routes(lines):
    text = "\n".join(lines)
    for word in ("FUSED launches=1 per=2,0", "FUSED launches=1 per=3,0", "FUSED launches=2 per=2,2", "SINGLE calls=1", "SINGLE calls=4", "wpb=8 dp=12", "wpb=4 dp=16"):
        assert word in text, word
    assert sum(" FUSED " in l for l in lines) >= 100
    for l in lines:
        f = dict(kv.split("=") for kv in l.split(":")[0].split())
        banks = [tuple(int(v) for v in b.split("/")) for b in f["banks"].split(",")]
        if (f["count"] == "1" or f["mis"] != "0" or int(f["streams"]) % 128 or int(f["ticks"]) <= 64 or f["dma"] == "0" or len({b[:2] for b in banks}) > 1 or
                banks[0][0] > max(MAX_N.values())):
            assert l.endswith(f" SINGLE calls={f['count']}"), l
    # the block moments are no reason to leave: fused half windows lie below their range, whatever the fit says
    assert any(" FUSED " in l and "/1/1/3" in l for l in lines)
    # config 3's shape, three outputs: 512 strips x 126 bands of the body in 16 128 blocks of four waves
    assert any(l.startswith("count=3 streams=65536 ticks=4096 ") and l.endswith("head=64 body=4032 wpb=4 dp=16 strips=512 bands=126 group=128 total=64512 grid=16128") for l in lines)
