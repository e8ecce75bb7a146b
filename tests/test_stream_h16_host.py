"""savgol_streambank_push_block_h16 on a CPU: the symbol and its ctypes binding, the refusals that need no device, and the route every call takes.

csrc/sg_stream_host.hpp (block_plan_h16) is built with plain g++ into tests/mock/stream_block_h16.cpp, which prints one line per call shape; every line is
held to the rule restated here from the call's contract (include/savgol_hip.h):
  TILES   streams % 128 == 0, ticks >= 64, both 16-bit bases 16-byte aligned, rows under the descriptor limit, and the fp32 call on ALIGNED buffers takes
          block-moment or LDS-DMA tiles (block_form, restated as in tests/stream_seams.py's expect(), the moment rule from sg_stream_host.hpp) -- then
          head = 64, body = ticks - 64, and the body's tiles are tile_geom(streams, 128, body, 32, the form's group, the form's waves per block);
  STAGED  everything else: one piece up to 2^24 stream-ticks, else chunks of max(64, (2^24 / streams) & ~63) ticks.
No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")
NAME = "savgol_streambank_push_block_h16"


def test_symbol_exported_and_bound(sg):
    assert NAME in sg.SIGNATURES
    fn = getattr(sg.lib(), NAME)
    assert len(fn.argtypes) == 7
    assert hasattr(sg.StreamBank, "push_block_h16")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == NAME for line in out.splitlines())
    # nothing of the new objects leaks past the version script
    assert not [line for line in out.splitlines() if "sg_bank_dma_h16" in line]


def test_refusals_that_need_no_device(sg):
    L = sg.lib()
    assert L.savgol_streambank_push_block_h16(None, 4096, sg.SAVGOL_HIP_F16, 8, 8192, sg.SAVGOL_HIP_F16, None) == -1
    assert NAME in sg.last_error() and "NULL pointer" in sg.last_error()


def shapes():
    """(n, fma, streams, ticks, misaligned, centre, moment_terms, dma_switch, moment_switch)"""
    out = []
    for n in (1, 12, 16, 17, 19, 20, 32):
        for fma in (0, 1):
            for streams in (1, 127, 128, 130, 256, 260, 2176, 16512):
                for ticks in (1, 63, 64, 65, 96, 97, 4096):
                    out.append((n, fma, streams, ticks, 0, 0, 2, 1, 1))
            for mis in (2, 8):                                             # either base 2 or 8 bytes off: the or of the low four bits
                for ticks in (64, 97):
                    out.append((n, fma, 256, ticks, mis, 0, 2, 1, 1))
            for dma, mom in ((0, 1), (1, 0), (0, 0)):
                out.append((n, fma, 256, 97, 0, 0, 2, dma, mom))
                out.append((n, fma, 2176, 4096, 0, 1, 2, dma, mom))
            for centre, terms in ((0, 0), (0, 1), (0, 3), (1, 2), (1, 3)):  # the fit's answer; quadratic taps summing to zero keep the tap-by-tap tiles
                out.append((n, fma, 2176, 160, 0, centre, terms, 1, 1))
    # over 2^24 stream-ticks: staged shapes in chunks, a tile shape in one piece whatever its size
    out += [(16, 1, 130, 129100, 0, 1, 2, 1, 1), (16, 0, 1, (1 << 24) + 1, 0, 0, 2, 1, 1), (8, 0, 777, 40000, 0, 0, 2, 1, 1),
            (8, 0, 1 << 25, 3, 0, 0, 2, 1, 1), (16, 1, 65536, 4096, 0, 1, 2, 1, 1), (17, 0, 65536, 4096, 0, 0, 2, 1, 1), (12, 0, 130, 1 << 17, 2, 0, 0, 1, 1)]
    return out


def tile_geom(streams, strip_width, ticks, tr, group, wpb):
    strips = -(-streams // strip_width)
    bands = -(-ticks // tr)
    group = min(group, strips)
    total = -(-strips // group) * group * bands
    grid = 0 if total >= 0x7fffff00 else (-(-total // wpb) + 7) & ~7
    return strips, bands, group, total, grid


def rule(n, fma, streams, ticks, mis, centre, terms, dma, mom):
    form = None
    if dma and streams % 128 == 0 and streams * 4 < 0x7fffff00 and mis == 0 and ticks >= 64:
        if fma and mom and 12 <= n <= 20 and terms > 0 and not (centre and terms >= 3):
            form = "MOMENT_TILES"
        elif n <= 16 or fma or n >= 20:
            form = "DMA_TILES"
    if form:
        if form == "MOMENT_TILES":
            wpb, group = 8, min(64, max(16, streams // 128 // 4))
        else:
            wpb, group = (8 if 5 < n <= 11 and fma else 4), 128
        if tile_geom(streams, 128, ticks, 32, group, wpb)[4] == 0:
            form = None
    head = f"n={n} fma={fma} streams={streams} ticks={ticks} mis={mis} centre={centre} terms={terms} dma={dma} mom={mom}:"
    if form:
        line = f"{head} TILES {form} head=64 body={ticks - 64} wpb={wpb}"
        if ticks > 64:
            line += " strips=%d bands=%d group=%d total=%d grid=%d" % tile_geom(streams, 128, ticks - 64, 32, group, wpb)
        return line
    chunk = ticks if streams * ticks <= 1 << 24 else max(64, ((1 << 24) // streams) & ~63)
    parts = [min(chunk, ticks - done) for done in range(0, ticks, chunk)] if ticks // chunk < 100000 else None
    if parts is None:                                                      # very many chunks: arithmetic instead of a list
        count = -(-ticks // chunk)
        last = ticks - (count - 1) * chunk
        shown = [chunk, chunk, chunk, last]
    else:
        count = len(parts)
        shown = parts[:3] + ([parts[-1]] if count > 3 else [])
    return f"{head} STAGED chunks={','.join(str(p) for p in shown)} count={count}"


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("stream_block_h16")), "stream_block_h16")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "stream_block_h16.cpp")],
                   check=True)
    text = "".join(" ".join(str(v) for v in shape) + "\n" for shape in shapes())
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def test_every_plan_follows_the_rule(lines):
    want = [rule(*shape) for shape in shapes()]
    assert len(lines) == len(want)
    bad = [(got, exp) for got, exp in zip(lines, want) if got != exp]
    for got, exp in bad[:8]:
        print(f"rule: {exp}\nplan: {got}")
    assert not bad, f"{len(bad)} of {len(want)} plans differ from the rule"


def test_the_table_takes_both_routes_and_both_forms(lines):
    text = "\n".join(lines)
    for word in ("TILES MOMENT_TILES", "TILES DMA_TILES", "STAGED chunks=", "body=0 wpb", "count=1\n"):
        assert word in text, word
    chunked = [l for l in lines if " STAGED " in l and not l.endswith("count=1")]
    assert len(chunked) >= 4
    # the GPU test's chunked case (tests/test_gpu_stream_h16.py): 130 streams, chunks of (2^24 / 130) & ~63 = 129024 ticks
    assert any(l.startswith("n=16 fma=1 streams=130 ticks=129100 ") and l.endswith("chunks=129024,76 count=2") for l in lines)
    # a pointer off by 2 or by 8 bytes, an odd stream count, 63 ticks, a bank whose fp32 call walks (bit-exact, n = 17 and 19): all staged
    for l in lines:
        f = dict(kv.split("=") for kv in l.split(":")[0].split())
        if f["mis"] != "0" or int(f["streams"]) % 128 or int(f["ticks"]) < 64 or (f["fma"] == "0" and f["n"] in ("17", "19")) or f["dma"] == "0":
            assert " STAGED " in l, l
