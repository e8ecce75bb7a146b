"""CPU-side checks of the int16-storage 1-D batch call (savgol_apply[_valid]_batch_i16): both symbols are bound with their arity and the storage
constant exported, every refusal returns -1 with its text before any device call (fake device addresses) and the documented first fault wins, the
call fails loudly without a device, apply_tensor_i16 refuses what it does not serve, the library's 71 new kernels carry no private segment, and --
csrc/sg_api_1d.cpp built against the launch recorder plus tests/mock/launch_i16_mock.cpp -- what the route enqueues is the job of the fp32
narrow-tile call on the widened input, field for field.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from tests.test_launch_record_1d import CSRC, GOLDEN, HIP_HEADER, ROCM, Recorder, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("savgol_apply_batch_i16", "savgol_apply_valid_batch_i16")
F32, F16, BF16, I16 = 0, 1, 2, 3
REF, PLAIN, NARROW, WIDE, CLE, AWARE, M64 = 1, 2, 4, 8, 16, 32, 64

# fake device addresses: the checks run before anything touches them
IN, OUT = 0x100000000000, 0x200000000000


def call(sg, name, f, d_in=IN, d_out=OUT, out_type=I16, channels=4, length=1000, in_ld=None, out_ld=None, flags=0):
    return getattr(sg.lib(), name)(None if f is None else f.ptr, d_in, d_out, out_type, channels, length,
                                   length if in_ld is None else in_ld, length if out_ld is None else out_ld, flags, None)


def test_i16_symbols_bound(sg):
    for name in NAMES:
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == 10
    assert sg.SAVGOL_HIP_I16 == 3
    assert "i16" not in sg._STORAGE and 3 not in sg._STORAGE.values()


@pytest.mark.parametrize("name", NAMES)
def test_i16_refusals_need_no_device(sg, name):
    f = sg.Filter(5, 2, 0)
    out_len = 990 if name == NAMES[1] else 1000                    # VALID: the output row is length - 2n long
    cases = [
        (dict(flags=REF), "SAVGOL_BATCH_REFERENCE_SUMMATION is not served"),
        (dict(flags=WIDE), "SAVGOL_BATCH_TILE_WIDE is not served"),
        (dict(flags=WIDE | NARROW), "SAVGOL_BATCH_TILE_WIDE is not served"),
        (dict(flags=AWARE), "belong to other calls"),
        (dict(flags=M64), "belong to other calls"),
        (dict(flags=0x1000), "bad flags 0x1000"),
        (dict(out_type=F16), "output type f16 (1) is not served"),
        (dict(out_type=BF16), "output type bf16 (2) is not served"),
        (dict(out_type=7), "output type unknown (7) is not served"),
        (dict(out_type=-1), "output type unknown (-1) is not served"),
        (dict(f=None), "NULL pointer"),
        (dict(d_in=None), "NULL pointer"),
        (dict(d_out=None), "NULL pointer"),
        (dict(length=10), "data length (10) < window size (11)"),
        (dict(length=(1 << 30) + 1, channels=1), "channels longer than 2^30 samples"),
        (dict(in_ld=999), "row pitch smaller than the row"),
        (dict(out_ld=500), "row pitch smaller than the row"),
        # shared bytes, compared byte-wise with element sizes 2 -> 2 or 4
        (dict(d_out=IN), "d_in and d_out overlap"),                                          # in place
        (dict(d_out=IN + 2), "d_in and d_out overlap"),                                       # shifted by one element
        (dict(d_out=IN + 4 * 1000 * 2 - 2), "d_in and d_out overlap"),                        # the input's last element
        (dict(d_out=IN - 3 * 1000 * 4 - out_len * 4 + 4, out_type=F32), "d_in and d_out overlap"),   # an fp32 output ending one element into the input
        (dict(d_in=IN, in_ld=2000, d_out=IN + 2 * 999, out_ld=2000), "d_in and d_out overlap"),    # interleaved rows, one byte pair shared
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc = call(sg, name, kw.pop("f", f), **kw)
        assert rc == -1, (text, rc)
        assert text in sg.last_error(), (text, sg.last_error())
        assert name in sg.last_error()
    if name == NAMES[1]:
        assert call(sg, name, f, out_ld=989) == -1 and "row pitch smaller than the row" in sg.last_error()
    if sg.device_count() == 0:
        # an fp32 output that ends exactly where the input begins shares nothing with it: the checks pass
        assert call(sg, name, f, d_out=IN - 3 * 1000 * 4 - out_len * 4, out_type=F32) == -1 and "no usable HIP device" in sg.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_i16_first_fault_in_order_wins(sg, name):
    """two faults in one call: the one that comes first in the documented order (include/savgol_hip.h) is reported"""
    f = sg.Filter(5, 2, 0)
    cases = [
        (dict(flags=REF | WIDE), "REFERENCE_SUMMATION is not served"),                        # 1: within the flags
        (dict(flags=WIDE | M64), "TILE_WIDE is not served"),
        (dict(flags=AWARE | 0x1000), "belong to other calls"),
        (dict(flags=0x1000, out_type=F16), "bad flags 0x1000"),                               # 1 before 2
        (dict(out_type=F16, d_in=None), "output type f16"),                                   # 2 before 3
        (dict(f=None, length=10), "NULL pointer"),                                            # 3: NULL first
        (dict(length=10, in_ld=5), "data length (10) < window size (11)"),                    #    then the length
        (dict(length=(1 << 30) + 1, in_ld=100, channels=1), "channels longer than 2^30 samples"),
        (dict(in_ld=999, d_out=IN), "row pitch smaller than the row"),                        # 3 before 4
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc = call(sg, name, kw.pop("f", f), **kw)
        assert rc == -1, (text, rc)
        assert text in sg.last_error(), (text, sg.last_error())
        assert name in sg.last_error()
    # zero channels: the argument checks pass and nothing is enqueued, whatever the buffers share
    assert call(sg, name, f, channels=0) == 0
    assert call(sg, name, f, channels=0, d_out=IN) == 0


@pytest.mark.parametrize("name", NAMES)
def test_i16_interleaved_rows_are_not_an_overlap(sg, name):
    """in = buf[:, 0, :], out = buf[:, 1, :] with equal BYTE pitches touch no common byte: the argument checks pass and the call gets as far as the device"""
    f = sg.Filter(5, 2, 0)
    if sg.device_count() == 0:
        assert call(sg, name, f, d_in=IN, in_ld=2000, d_out=IN + 2 * 1000, out_ld=2000) == -1
        assert "no usable HIP device" in sg.last_error()
        assert call(sg, name, f, d_in=IN, in_ld=4000, d_out=IN + 2 * 1000, out_ld=2000, out_type=F32) == -1      # 8000-byte pitch: 2000 + 4000 bytes per row pair
        assert "no usable HIP device" in sg.last_error()
    # the same rows one element closer share a byte pair
    assert call(sg, name, f, d_in=IN, in_ld=4000, d_out=IN + 2 * 999, out_ld=2000, out_type=F32) == -1
    assert "d_in and d_out overlap" in sg.last_error()


def test_i16_no_cpu_fallback_without_device(sg):
    """With valid arguments and no GPU the call must FAIL, not compute on the host"""
    if sg.device_count() > 0:
        pytest.skip("a GPU is present")
    f = sg.Filter(5, 4, 1)
    for name in NAMES:
        for ot in (I16, F32):
            assert call(sg, name, f, out_type=ot) == -1
            assert "no usable HIP device" in sg.last_error()
    with pytest.raises(RuntimeError):
        f.apply_batch_i16(IN, OUT, 4, 1000, out_dtype="f32")
    with pytest.raises(ValueError):
        f.apply_batch_i16(IN, OUT, 4, 1000, out_dtype="f16")


def test_apply_tensor_i16_refuses_unserved_dtypes(sg):
    import torch
    f = sg.Filter(5, 2, 0)
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.uint8, torch.float64):
        with pytest.raises(TypeError):
            f.apply_tensor_i16(torch.zeros((2, 100), dtype=dt))
    for out in (torch.float16, torch.bfloat16, torch.int32, torch.float64):
        with pytest.raises(TypeError):
            f.apply_tensor_i16(torch.zeros((2, 100), dtype=torch.int16), out_dtype=out)
    # the float calls keep refusing int16
    with pytest.raises(TypeError):
        f.apply_tensor(torch.zeros((2, 100), dtype=torch.int16))


def test_i16_kernels_in_the_library_have_no_private_segment():
    lib = os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")
    if not (os.path.exists(lib) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("library or llvm-readelf not present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), lib, "sg1d_i16_"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    plain, moment = {}, {}
    for line in out.stdout.splitlines():
        m = re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) spill\s+(\d+) lds\s+(\d+)\s+.*sg1d_i16_(momenth_)?kernel<(\d+)(?:, (\d+))?>", line)
        if m:
            row = (int(m.group(3)), int(m.group(4)), int(m.group(1)), int(m.group(5)))
            if m.group(6):
                moment[(int(m.group(7)), int(m.group(8)))] = row
            else:
                plain[int(m.group(7))] = row
    assert set(plain) == set(range(1, 33)), sorted(plain)
    assert set(moment) == {(n, t) for n in range(20, 33) for t in (3, 5, 7)}, sorted(moment)
    for key, (scratch, spill, vgpr, lds) in list(plain.items()) + list(moment.items()):
        assert scratch == 0 and spill == 0, (key, scratch, spill)
        assert vgpr <= 128, (key, vgpr)                      # 4 waves per SIMD, as the fp32 kernels of the narrow tile
    for n, (_, _, _, lds) in plain.items():
        assert lds <= 4 * 9728, (n, lds)                     # four waves' fp32 slabs: the fp32 narrow tile's LDS, nothing added


# ---- what the route enqueues: csrc/sg_api_1d.cpp against the launch recorder + the mock of the new launcher ----------------------------------------
STREAM = 0x5700
VEC_IN, VEC_OUT = 1 << 9, 1 << 10
I16_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p]


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    if not os.path.exists(HIP_HEADER):
        pytest.skip("hip/hip_runtime_api.h is not installed")
    tmp = str(tmp_path_factory.mktemp("launch_recorder_i16"))
    so = os.path.join(tmp, "libsg_launch_recorder_i16.so")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]
    wobj = os.path.join(tmp, "sg_weights.o")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", *inc, "-c", os.path.join(CSRC, "sg_weights.c"), "-o", wobj], check=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wl,-z,defs", *inc, "-o", so, os.path.join(CSRC, "sg_api_1d.cpp"),
                    os.path.join(CSRC, "sg_k1d_moment_fit.cpp"), os.path.join(ROOT, "tests", "mock", "launch_recorder_1d.cpp"),
                    os.path.join(ROOT, "tests", "mock", "launch_i16_mock.cpp"), wobj, "-lm", "-lpthread"], check=True)
    lib = load(so)
    for name in NAMES:
        getattr(lib, name).argtypes = I16_ARGS
    return Recorder(lib)


def record(R, variant, f, ot=I16, ch=4, L=1000, flags=0, d_in=IN, d_out=OUT, in_ld=None, out_ld=None, f32=False):
    """one call on a fresh record -> (rc, error text, the record's launcher lines)"""
    R.begin()
    v = "_valid" if variant == "valid" else ""
    in_ld, out_ld = L if in_ld is None else in_ld, L if out_ld is None else out_ld
    if f32:
        rc = R.call(f"savgol_apply{v}_batch_f32_ex", f, d_in, d_out, ch, L, in_ld, out_ld, flags, STREAM)
    else:
        rc = R.call(f"savgol_apply{v}_batch_i16", f, d_in, d_out, ot, ch, L, in_ld, out_ld, flags, STREAM)
    log, _ = R.end()
    lines = [l for l in log.splitlines() if l and not l.startswith(("call ", "-> ", "part "))]
    return rc, R.lib.savgol_hip_last_error().decode(), lines


def fields(line):
    return dict(re.findall(r"(\w+)=([^\s{}]+)", line))


def table_address(name):
    """the recorder's name of an uploaded table -> the address its ctx_table hands out for it (launch_recorder_1d.cpp); 'null' -> 0"""
    if name == "null":
        return 0
    m = re.fullmatch(r"table\(0x([0-9a-f]+),([0-9a-f]{16}),(\d+)\)", name)
    assert m, name
    salt, d = int(m.group(1), 16), int(m.group(2), 16)
    return 0x700000000000 + ((((d ^ ((salt * 0x9E3779B97F4A7C15) & (2 ** 64 - 1))) & 0xffffffffff) << 4))


# every Job1D field but the pointers and the flags (compared apart: the alignment bits depend on the element size)
SCALARS = ("n", "grid", "stream", "in_ld", "out_ld", "length", "tiles_per_channel", "total_tiles", "tpc_magic", "tpc_shift", "store_lo", "store_hi", "out_shift",
           "dt_inv", "edge_items", "phase", "tpc_all", "xcd_chunk_log2", "centre_sum")
FILTERS = ((4, 0, 1.0), (3, 1, 0.5), (4, 2, 0.5))                  # (poly_order, derivative, time_step): d = 0, 1, 2


def assert_same_job(lines, want, ot, ch, L, d_in=IN, d_out=OUT):
    """`lines`: the int16 route's record; `want`: the fp32 narrow-tile call's on the same shape"""
    assert len(lines) == len(want) >= 1, (lines, want)
    ob = 4 if ot == F32 else 2
    for line, wline in zip(lines, want):
        g, w = fields(line), fields(wline)
        assert line.startswith("i16 ")
        moment = wline.startswith("f32_momenth_t")
        assert moment or (wline.startswith("f32_g") and w["wide"] == "0"), wline
        # the kernel family, and what it reads its weights from
        if moment:
            assert int(g["moment_terms"]) == int(wline.split(" ", 1)[0][len("f32_momenth_t"):])
            assert int(g["table"], 16) == table_address(w["table"]) != 0
        else:
            assert g["moment_terms"] == "0" and g["table"] == "0x0" and g["taps"] == w["taps"]
        assert int(g["out_type"]) == ot
        assert {k: g[k] for k in SCALARS} == {k: w[k] for k in SCALARS}, (line, wline)
        assert int(g["flags"], 16) & ~(VEC_IN | VEC_OUT) == int(w["flags"], 16) & ~(VEC_IN | VEC_OUT), (line, wline)
        assert int(g["edges"], 16) == table_address(w["edges"])
        assert (int(g["stash"], 16), int(g["ends"], 16), int(g["edge_stash"], 16)) == (0, 0, 0) and (w["stash"], w["ends"], w["edge_stash"]) == ("null",) * 3
        # the same rows: the fp32 call's offsets are in 4-byte elements, this call's in its own
        win, wout = re.fullmatch(r"in\+(\d+)", w["in"]), re.fullmatch(r"out\+(\d+)", w["out"])
        assert win and wout, wline
        assert (int(g["in"], 16) - d_in) * 4 == int(win.group(1)) * 2 and (int(g["out"], 16) - d_out) * 4 == int(wout.group(1)) * ob, (line, wline)


@pytest.mark.parametrize("variant,mode", (("full", 0), ("full", 1), ("full", 2), ("full", 3), ("valid", 0)))
@pytest.mark.parametrize("n", (5, 19, 20, 32))
def test_the_job_is_the_fp32_narrow_tile_calls(rec, n, variant, mode):
    took_moments = set()
    for m, d, dt in FILTERS:
        f = rec.filt(n, m, d, dt, mode)
        for ot in (I16, F32):
            for flags in (0, PLAIN, CLE, NARROW):
                for ch, L in ((4, 1000), (3, 9004)):
                    rc, err, lines = record(rec, variant, f, ot, ch, L, flags)
                    assert rc == 0, err
                    rc, err, want = record(rec, variant, f, ot, ch, L, flags | NARROW, f32=True)
                    assert rc == 0, err
                    assert len(lines) == 1
                    assert_same_job(lines, want, ot, ch, L)
                    if fields(lines[0])["moment_terms"] != "0":
                        took_moments.add((d, flags))
                    if variant == "valid":
                        assert fields(lines[0])["edge_items"] == "0" and fields(lines[0])["out_shift"] == str(n)
                    # both buffers at 16-byte aligned bases with pitches that are multiples of four: vectors, unless VALID shifts the output by an odd n
                    vec = VEC_IN | (VEC_OUT if variant == "full" or n % 4 == 0 else 0)
                    assert int(fields(lines[0])["flags"], 16) & (VEC_IN | VEC_OUT) == vec == int(fields(want[0])["flags"], 16) & (VEC_IN | VEC_OUT)
    # block moments from half window 20 for poly_order >= 2 and derivative <= 1, unless PLAIN_SUMMATION asks otherwise (takes_moment32)
    assert took_moments == ({(0, 0), (0, CLE), (0, NARROW), (1, 0), (1, CLE), (1, NARROW)} if n >= 20 else set())


@pytest.mark.parametrize("variant", ("full", "valid"))
@pytest.mark.parametrize("n", (5, 19, 20, 32))
def test_30_million_short_channels_split_over_channels(rec, n, variant):
    """more than one channel group: the launches of the fp32 call, one for one"""
    CH, L = 30000000, 100
    for m, d, dt in FILTERS[:2]:
        f = rec.filt(n, m, d, dt, 0)
        for ot in (I16, F32):
            rc, err, lines = record(rec, variant, f, ot, CH, L)
            assert rc == 0, err
            rc, err, want = record(rec, variant, f, ot, CH, L, NARROW, f32=True)
            assert rc == 0, err
            per_launch = 4 * ((1 << 24) - 8) // 3                  # MAX_TILES_PER_LAUNCH over one tile and two edge items per channel, as the fp32 call counts
            assert len(lines) == -(-CH // per_launch) == 2 and int(fields(lines[0])["total_tiles"]) == per_launch
            assert_same_job(lines, want, ot, CH, L)
            assert sum(int(fields(l)["total_tiles"]) for l in lines) == CH


def test_alignment_is_counted_in_the_buffers_own_elements(rec):
    """JOB_VEC_IN / JOB_VEC_OUT: 8-byte groups for int16 rows, 16-byte groups for fp32 output rows"""
    f = rec.filt(4, 2, 0)
    for ot in (I16, F32):
        ob = 4 if ot == F32 else 2
        for d_in, in_ld, d_out, out_ld, vin, vout in ((IN + 8, 1000, OUT + 8, 1000, True, ob == 2),
                                                      (IN + 8, 1000, OUT + 16, 1000, True, True),
                                                      (IN + 2, 1000, OUT + ob, 1000, False, False),
                                                      (IN + 4, 1000, OUT + 4, 1000, False, False),
                                                      (IN, 1001, OUT, 1003, False, False),
                                                      (IN, 1004, OUT, 1002, True, False)):
            rc, err, lines = record(rec, "full", f, ot, 3, 1000, d_in=d_in, d_out=d_out, in_ld=in_ld, out_ld=out_ld)
            assert rc == 0 and len(lines) == 1, err
            flags = int(fields(lines[0])["flags"], 16)
            assert (bool(flags & VEC_IN), bool(flags & VEC_OUT)) == (vin, vout), (d_in - IN, in_ld, d_out - OUT, out_ld, lines)
    # VALID shifts the output by n elements: only a multiple of four keeps the groups aligned
    for n, vout in ((4, True), (5, False), (8, True)):
        rc, err, lines = record(rec, "valid", rec.filt(n, 2, 0), I16, 3, 1000)
        assert rc == 0, err
        assert bool(int(fields(lines[0])["flags"], 16) & VEC_OUT) == vout


def test_the_existing_record_build_refuses_without_the_launcher(tmp_path):
    """sg_api_1d.cpp linked WITHOUT an object that defines the launcher (the build of tests/test_launch_record_1d.py): the symbol is weak, the link
    closes under -z defs, the call refuses with a text instead of calling through a null pointer, and the record of every other route is the golden one"""
    if not os.path.exists(HIP_HEADER):
        pytest.skip("hip/hip_runtime_api.h is not installed")
    from tests.test_launch_record_1d import build, run_cases
    lib = load(build(str(tmp_path)))
    R = Recorder(lib)
    for name in NAMES:
        getattr(lib, name).argtypes = I16_ARGS
    for variant, name in zip(("full", "valid"), NAMES):
        rc, err, lines = record(R, variant, R.filt(4, 2, 0))
        assert rc == -1 and "object not linked" in err and name in err and not lines
        # the argument checks still come first
        rc, err, lines = record(R, variant, R.filt(4, 2, 0), d_out=IN)
        assert rc == -1 and "d_in and d_out overlap" in err and not lines
        rc, err, lines = record(R, variant, R.filt(4, 2, 0), ch=0)
        assert rc == 0 and not lines
    with open(GOLDEN) as fh:
        want = {line.split("\t", 1)[0]: line.rstrip("\n") for line in fh if line.strip()}
    got = run_cases(lib)
    assert set(got) == set(want) and not [cid for cid in got if got[cid][0] != want[cid]]
