"""CPU-side checks of the fused multi-output 1-D call on int16 storage (savgol_apply[_valid]_multi_batch_i16): both symbols are bound with their
arity, every refusal returns -1 with its text before any device call (fake device addresses) and the documented first fault wins, the call fails
loudly without a device, apply_multi_tensor_i16 refuses what it does not serve, the library carries exactly the 64 new kernels without a private
segment, and -- csrc/sg_api_1d.cpp built against the launch recorder plus tests/mock/launch_i16_mock.cpp and tests/mock/launch_multi_i16_mock.cpp --
what the route enqueues: which launcher, how many launches, the channel split, the edge items, and the job of the fp32 fused call on the widened
input field for field.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from tests.test_launch_record_1d import CSRC, HIP_HEADER, ROCM, Recorder, SavgolFilter, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("savgol_apply_multi_batch_i16", "savgol_apply_valid_multi_batch_i16")
F32, F16, BF16, I16 = 0, 1, 2, 3
OUT_TYPES = (I16, F32)
REF, PLAIN, NARROW, WIDE, CLE, AWARE, M64 = 1, 2, 4, 8, 16, 32, 64

# fake device addresses: the checks run before anything touches them
IN, OUT0, OUT1, OUT2, OUT3 = 0x100000000000, 0x200000000000, 0x210000000000, 0x220000000000, 0x230000000000
OUTS = (OUT0, OUT1, OUT2, OUT3)


def call(sg, name, filters, d_in=IN, d_outs=None, out_type=I16, channels=4, length=1000, in_ld=None, out_ld=None, flags=0, count=None):
    F = C.POINTER(sg.SavgolFilter)
    fs = None if filters is None else (F * max(len(filters), 1))(*[f.ptr if f is not None else F() for f in filters])
    if d_outs is None and filters is not None:
        d_outs = list(OUTS[:len(filters)])
    outs = None if d_outs is None or d_outs == "NULL" else (C.c_void_p * max(len(d_outs), 1))(*d_outs)
    count = len(filters) if count is None else count
    return getattr(sg.lib(), name)(fs, count, d_in, outs, out_type, channels, length, length if in_ld is None else in_ld,
                                   length if out_ld is None else out_ld, flags, None)


def test_multi_i16_symbols_bound(sg):
    for name in NAMES:
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == 11
    assert sg.SAVGOL_MULTI_MAX_FILTERS == 4 and sg.SAVGOL_HIP_I16 == 3


@pytest.mark.parametrize("name", NAMES)
def test_multi_i16_refusals_need_no_device(sg, name):
    a, b, c = sg.Filter(5, 2, 0), sg.Filter(5, 3, 1), sg.Filter(5, 4, 2)
    bad = sg.Filter(5, 3, 1)
    bad.ptr.contents.window_size = 13
    cases = [
        # those of the int16 single call, in its words
        (dict(flags=REF), "SAVGOL_BATCH_REFERENCE_SUMMATION is not served on int16 storage"),
        (dict(flags=WIDE), "SAVGOL_BATCH_TILE_WIDE is not served on int16 storage"),
        (dict(flags=WIDE | NARROW), "SAVGOL_BATCH_TILE_WIDE is not served"),
        (dict(flags=AWARE), "belong to other calls"),
        (dict(flags=M64), "belong to other calls"),
        (dict(flags=0x1000), "bad flags 0x1000"),
        (dict(out_type=F16), "output type f16 (1) is not served"),
        (dict(out_type=BF16), "output type bf16 (2) is not served"),
        (dict(out_type=7), "output type unknown (7) is not served"),
        (dict(out_type=-1), "output type unknown (-1) is not served"),
        (dict(length=(1 << 30) + 1, channels=1), "channels longer than 2^30 samples"),
        # those of the multi-output call
        (dict(filters=None, d_outs=[OUT0], count=1), "NULL pointer"),
        (dict(d_in=None), "NULL pointer"),
        (dict(d_outs="NULL"), "NULL pointer"),
        (dict(filters=[a, None]), "NULL pointer (filters[1] / d_outs[1])"),
        (dict(d_outs=[OUT0, None]), "NULL pointer (filters[1] / d_outs[1])"),
        (dict(filters=[a, bad]), "not a valid SavgolFilter"),
        (dict(count=0), "count 0 outside 1..4"),
        (dict(filters=[a, b, c, a, b], d_outs=[OUT0, OUT1, OUT2, OUT3, OUT3 + (1 << 36)]), "count 5 outside 1..4"),
        (dict(filters=[a, sg.Filter(6, 3, 1)]), "half_window"),
        (dict(filters=[a, sg.Filter(5, 3, 1, 1.0, sg.SAVGOL_BOUNDARY_REFLECT)]), "boundary"),
        (dict(length=10), "data length (10) < window size (11)"),
        (dict(in_ld=999), "row pitch smaller than the row"),
        (dict(out_ld=500), "row pitch smaller than the row"),
        # shared bytes, compared byte-wise
        (dict(d_outs=[OUT0, IN]), "d_outs[1] overlaps d_in"),                                       # in place
        (dict(d_outs=[IN + 2, OUT1]), "d_outs[0] overlaps d_in"),                                    # shifted by one element
        (dict(d_outs=[OUT0, IN + 4 * 1000 * 2 - 2]), "d_outs[1] overlaps d_in"),                     # one shared element: the input's last
        (dict(d_outs=[IN - 3 * 1000 * 4 - 4, OUT1], out_type=F32), "d_outs[0] overlaps d_in"),       # an fp32 output whose last row ends inside the input's first element
        (dict(in_ld=2000, out_ld=2000, d_outs=[OUT0, IN + 2 * 999]), "d_outs[1] overlaps d_in"),     # interleaved rows, one element shared
        (dict(d_outs=[OUT0, OUT0 + 400]), "d_outs[0] and d_outs[1] overlap"),
        (dict(filters=[a, b, c], d_outs=[OUT0, OUT1, OUT0]), "d_outs[0] and d_outs[2] overlap"),
        (dict(filters=[a, b, c], d_outs=[OUT0, OUT1, OUT1 + 4 * 3 * 1000], out_type=F32), "d_outs[1] and d_outs[2] overlap"),
        (dict(count=1, d_outs=[IN + 2, OUT1]), "d_outs[0] overlaps d_in"),                           # count 1 refuses in the call's own words too
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc = call(sg, name, kw.pop("filters", [a, b]), **kw)
        assert rc == -1, (text, rc)
        assert text in sg.last_error(), (text, sg.last_error())
        assert name in sg.last_error()
    if name == NAMES[1]:
        # VALID: the output row is length - 2n long
        assert call(sg, name, [a, b], out_ld=989) == -1 and "row pitch smaller than the row" in sg.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_multi_i16_first_fault_in_order_wins(sg, name):
    """two faults in one call: the one that comes first in the documented order (include/savgol_hip.h) is reported"""
    a, b = sg.Filter(5, 2, 0), sg.Filter(5, 3, 1)
    other_n, other_b = sg.Filter(6, 3, 1), sg.Filter(5, 3, 1, 1.0, sg.SAVGOL_BOUNDARY_REFLECT)
    cases = [
        (dict(flags=REF | WIDE), "REFERENCE_SUMMATION is not served"),                               # 1: within the flags
        (dict(flags=WIDE | M64), "TILE_WIDE is not served"),
        (dict(flags=WIDE | 0x1000), "TILE_WIDE is not served"),
        (dict(flags=M64 | 0x1000), "belong to other calls"),
        (dict(flags=0x1000, out_type=F16), "bad flags 0x1000"),                                      # 1 before 2
        (dict(out_type=F16, d_in=None), "output type f16"),                                          # 2 before 3
        (dict(d_in=None, count=0), "NULL pointer"),                                                  # 3 before 4
        (dict(count=7, filters=[a, None]), "count 7 outside 1..4"),                                  # 4 before 5
        (dict(filters=[a, None, other_n], d_outs=[OUT0, OUT1, OUT2]), "NULL pointer (filters[1]"),   # 5 before 6
        (dict(filters=[a, other_n, other_b], d_outs=[OUT0, OUT1, OUT2]), "half_window"),             # 6: k ascending
        (dict(filters=[a, other_b, other_n], d_outs=[OUT0, OUT1, OUT2]), "boundary"),
        (dict(filters=[a, other_n], length=10), "half_window"),                                      # 6 before 7
        (dict(length=10, in_ld=5), "data length (10) < window size (11)"),                           # 7: length first
        (dict(length=(1 << 30) + 1, in_ld=100, channels=1), "channels longer than 2^30 samples"),
        (dict(in_ld=999, d_outs=[OUT0, IN]), "row pitch smaller than the row"),                      # 7 before 8
        (dict(filters=[a, b, a], d_outs=[OUT0, OUT0, IN]), "d_outs[0] and d_outs[1] overlap"),       # 8: k ascending
        (dict(filters=[a, b, a], d_outs=[OUT0, IN, OUT0]), "d_outs[1] overlaps d_in"),
        (dict(filters=[a, b, a], d_outs=[OUT0, OUT1, IN], out_type=F32), "d_outs[2] overlaps d_in"),
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc = call(sg, name, kw.pop("filters", [a, b]), **kw)
        assert rc == -1, (text, rc)
        assert text in sg.last_error(), (text, sg.last_error())
        assert name in sg.last_error()
    # zero channels: the argument checks pass and nothing is enqueued, whatever the buffers share
    assert call(sg, name, [a, b], channels=0) == 0
    assert call(sg, name, [a, b], channels=0, d_outs=[IN, IN]) == 0


def test_multi_i16_no_cpu_fallback_without_device(sg):
    """With valid arguments and no GPU the call must FAIL, not compute on the host"""
    if sg.device_count() > 0:
        pytest.skip("a GPU is present")
    fs = [sg.Filter(5, 4, d) for d in (0, 1, 2, 0)]
    for name in NAMES:
        for ot in OUT_TYPES:
            for count in (1, 2, 3, 4):
                assert call(sg, name, fs[:count], out_type=ot) == -1
                assert "no usable HIP device" in sg.last_error()
        # interleaved rows of equal byte pitch share nothing: the checks pass
        assert call(sg, name, fs[:2], in_ld=2000, out_ld=2000, d_outs=[IN + 2 * 1000, OUT0]) == -1
        assert "no usable HIP device" in sg.last_error()
        assert call(sg, name, fs[:2], in_ld=4000, out_ld=2000, d_outs=[IN + 2 * 1000, OUT0], out_type=F32) == -1      # 8000-byte pitch: 2000 + 4000 bytes per row pair
        assert "no usable HIP device" in sg.last_error()
        # an fp32 output that ends exactly where the input begins shares nothing with it
        out_len = 990 if name == NAMES[1] else 1000
        assert call(sg, name, fs[:2], d_outs=[IN - 3 * 1000 * 4 - out_len * 4, OUT1], out_type=F32) == -1
        assert "no usable HIP device" in sg.last_error()
    with pytest.raises(RuntimeError):
        sg.apply_multi_batch_i16(fs[:3], IN, list(OUTS[:3]), 4, 1000, out_dtype="f32")
    with pytest.raises(ValueError):
        sg.apply_multi_batch_i16(fs[:3], IN, list(OUTS[:3]), 4, 1000, out_dtype="f16")


def test_apply_multi_tensor_i16_refuses_unserved_dtypes(sg):
    import torch
    fs = [sg.Filter(5, 2, 0), sg.Filter(5, 3, 1)]
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.float64):
        with pytest.raises(TypeError):
            sg.apply_multi_tensor_i16(fs, torch.zeros((2, 100), dtype=dt))
    for out in (torch.float16, torch.bfloat16, torch.int32):
        with pytest.raises(TypeError):
            sg.apply_multi_tensor_i16(fs, torch.zeros((2, 100), dtype=torch.int16), out_dtype=out)
    # the float call keeps refusing int16
    with pytest.raises(TypeError):
        sg.apply_multi_tensor(fs, torch.zeros((2, 100), dtype=torch.int16))


def test_multi_i16_kernels_in_the_library_have_no_private_segment():
    lib = os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")
    if not (os.path.exists(lib) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("library or llvm-readelf not present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), lib, "sg1d_multi_i16_kernel"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) spill\s+(\d+) lds\s+(\d+)\s+.*sg1d_multi_i16_kernel<(\d+), (\d+)>", line)
        if m:
            rows[(int(m.group(6)), int(m.group(7)))] = (int(m.group(3)), int(m.group(4)), int(m.group(1)), int(m.group(5)))
    assert set(rows) == {(n, k) for n in range(1, 33) for k in (2, 3)}, sorted(rows)
    for key, (scratch, spill, vgpr, lds) in rows.items():
        assert scratch == 0 and spill == 0, (key, scratch, spill)
        assert vgpr <= 256, (key, vgpr)                      # 2 waves per SIMD
        assert lds <= 4 * (9728 + 8192), (key, lds)          # sg1d_multi_kernel's: a slab and a result region per wave, two blocks per CU


# ---- what the route enqueues: csrc/sg_api_1d.cpp against the launch recorder + the mocks of the two int16 launchers ---------------------------------
STREAM = 0x5700
REC_BASES = (("in", IN), ("out", OUT0), ("out1", OUT1), ("out2", OUT2), ("out3", OUT3))
ARGS = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p]


def build_recorder(tmp, mocks):
    """csrc/sg_api_1d.cpp + the launch recorder + the given mock launchers -> the library's path"""
    so = os.path.join(tmp, "libsg_launch_recorder_multi_i16.so")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]
    wobj = os.path.join(tmp, "sg_weights.o")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", *inc, "-c", os.path.join(CSRC, "sg_weights.c"), "-o", wobj], check=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wl,-z,defs", *inc, "-o", so, os.path.join(CSRC, "sg_api_1d.cpp"),
                    os.path.join(CSRC, "sg_k1d_moment_fit.cpp"), os.path.join(ROOT, "tests", "mock", "launch_recorder_1d.cpp"),
                    *[os.path.join(ROOT, "tests", "mock", m) for m in mocks], wobj, "-lm", "-lpthread"], check=True)
    lib = load(so)
    for name in NAMES:
        getattr(lib, name).argtypes = ARGS
    return lib


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    if not os.path.exists(HIP_HEADER):
        pytest.skip("hip/hip_runtime_api.h is not installed")
    return Recorder(build_recorder(str(tmp_path_factory.mktemp("launch_recorder_multi_i16")), ("launch_i16_mock.cpp", "launch_multi_i16_mock.cpp")))


def record(R, variant, filters, outs, ot, ch=4, L=1000, flags=0, d_in=IN, in_ld=None, out_ld=None, f32=False):
    """one call on a fresh record -> (rc, error text, the record's launcher lines)"""
    FP = C.POINTER(SavgolFilter)
    fs = (FP * len(filters))(*filters)
    os_ = (C.c_void_p * len(outs))(*outs)
    R.begin()
    v = "_valid" if variant == "valid" else ""
    in_ld, out_ld = L if in_ld is None else in_ld, L if out_ld is None else out_ld
    if f32:
        rc = R.call(f"savgol_apply{v}_multi_batch_f32", fs, len(filters), d_in, os_, ch, L, in_ld, out_ld, flags, STREAM)
    else:
        rc = R.call(f"savgol_apply{v}_multi_batch_i16", fs, len(filters), d_in, os_, ot, ch, L, in_ld, out_ld, flags, STREAM)
    log, _ = R.end()
    lines = [l for l in log.splitlines() if l and not l.startswith(("call ", "-> ", "part "))]
    return rc, R.lib.savgol_hip_last_error().decode(), lines


def fields(line):
    """'name k=v ... [0]{k=v ...} ...' -> ({k: v} of the part before the outputs, [{k: v}] per output)"""
    head, *outs = re.split(r" \[\d\]\{", line)
    kv = lambda text: dict(re.findall(r"(\w+)=([^\s{}]+)", text))
    return kv(head), [kv(o) for o in outs]


MIX = ((2, 0, 1.0), (3, 1, 0.5), (4, 2, 0.5), (4, 0, 1.0))          # (poly_order, derivative, time_step) of outputs 0..3


@pytest.mark.parametrize("variant", ("full", "valid"))
def test_count_1_takes_the_int16_single_launcher_with_plain_summation(rec, variant):
    # n = 32, poly_order 4, smoothing: the default single call takes the block-moment kernels, PLAIN_SUMMATION the plain one (moment_terms = 0: the
    # launcher hands the job to the i16_g* objects)
    f = rec.filt(32, 4, 0)
    for ot in OUT_TYPES:
        for flags in (0, CLE, NARROW):
            rc, err, lines = record(rec, variant, [f], [OUT0], ot, flags=flags)
            assert rc == 0, err
            assert len(lines) == 1 and lines[0].startswith("i16 n=32 moment_terms=0 "), lines
            assert f" table=0x0 out_type={ot} " in lines[0]
            assert f"in=0x{IN:x} out=0x{OUT0:x} " in lines[0]
    # the control: the single call's own default at this shape is the block-moment kernel
    rec.lib.savgol_apply_batch_i16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p]
    rec.begin()
    assert rec.call("savgol_apply_batch_i16", f, IN, OUT0, I16, 4, 1000, 1000, 1000, 0, STREAM) == 0
    log, _ = rec.end()
    assert [l for l in log.splitlines() if l.startswith("i16 ")][0].split()[2] != "moment_terms=0"


@pytest.mark.parametrize("variant,mode", (("full", 0), ("full", 1), ("full", 300), ("valid", 0)))
@pytest.mark.parametrize("n", (4, 14, 15, 23, 32))
def test_counts_2_3_4_and_the_job_of_the_fp32_fused_call(rec, n, variant, mode):
    """count 2 / 3: one launch with that K; count 4: two launches of K = 2; the job is the fp32 fused call's under TILE_NARROW, field for field"""
    fs = [rec.filt(n, m, d, dt, mode) for m, d, dt in MIX]
    SCALARS = ("n", "grid", "nraw", "length", "tiles_per_channel", "total_tiles", "tpc_magic", "tpc_shift", "store_lo", "store_hi", "out_shift", "flags", "edge_items",
               "xcd_chunk_log2")
    for ot in OUT_TYPES:
        for count in (2, 3, 4):
            for flags in (0, CLE):
                for ch, L in ((4, 1000), (3, 9004)):
                    rc, err, lines = record(rec, variant, fs[:count], OUTS[:count], ot, ch, L, flags)
                    assert rc == 0, err
                    assert [l.split(" ", 1)[0] for l in lines] == ["multi_i16"] * (2 if count == 4 else 1), lines
                    rc, err, want = record(rec, variant, fs[:count], OUTS[:count], ot, ch, L, flags | NARROW, f32=True)
                    assert rc == 0 and len(want) == len(lines), (err, want)
                    for line, wline in zip(lines, want):
                        head, outs = fields(line)
                        whead, wouts = fields(wline)
                        K = 2 if count == 4 else count
                        assert int(head["k"]) == K and wline.startswith(f"multi{K}_g")
                        assert int(head["out_type"]) == ot
                        assert {k: head[k] for k in SCALARS} == {k: whead[k] for k in SCALARS}, (line, wline)
                        assert (int(head["in_ld"]), int(head["out_ld"])) == (L, L)
                        for o, w in zip(outs, wouts):
                            assert {k: o[k] for k in ("dt_inv", "centre_sum", "flags", "taps")} == {k: w[k] for k in ("dt_inv", "centre_sum", "flags", "taps")}
                            assert (o["has_edges"] == "1") == (w["edges"] != "null")
                        # the outputs in the launch's order (smoothing first) at the fp32 call's places, the input at its base
                        names = {f"0x{addr:x}": name + "+0" for name, addr in REC_BASES}
                        assert [names.get(o["out"], "null") for o in outs] == [w["out"] for w in wouts], (line, wline)
                        assert int(head["in"], 16) == IN
                        if variant == "valid":
                            assert head["edge_items"] == "0"
                    if count == 4:
                        assert [fields(l)[1][0]["out"] for l in lines] == [f"0x{OUT0:x}", f"0x{OUT3:x}"]       # (0, 1) then (3, 2): smoothing first within each


def test_alignment_is_counted_in_the_buffers_own_elements(rec):
    """JOB_VEC_IN / JOB_VEC_OUT: 8-byte groups for int16 rows, 16-byte groups for fp32 output rows"""
    VEC_IN, VEC_OUT = 1 << 9, 1 << 10
    fs = [rec.filt(4, 2, 0), rec.filt(4, 3, 1)]
    for ot in OUT_TYPES:
        ob = 4 if ot == F32 else 2
        for d_in, in_ld, outs, out_ld, vin, vout in ((IN + 8, 1000, (OUT0 + 8, OUT1 + 16), 1000, True, (ob == 2, True)),
                                                     (IN + 2, 1000, (OUT0 + ob, OUT1), 1000, False, (False, True)),
                                                     (IN + 4, 1000, (OUT0 + 4, OUT1), 1000, False, (False, True)),
                                                     (IN, 1001, (OUT0, OUT1), 1003, False, (False, False)),
                                                     (IN, 1004, (OUT0, OUT1), 1002, True, (False, False))):
            rc, err, lines = record(rec, "full", fs, outs, ot, 3, 1000, d_in=d_in, in_ld=in_ld, out_ld=out_ld)
            assert rc == 0 and len(lines) == 1, err
            head, o = fields(lines[0])
            assert bool(int(head["flags"], 16) & VEC_IN) == vin, lines
            assert tuple(bool(int(x["flags"], 16) & VEC_OUT) for x in o[:2]) == vout, lines


@pytest.mark.parametrize("variant", ("full", "valid"))
def test_30_million_short_channels_split_over_channels(rec, variant):
    CH, L = 30000000, 100
    MAX_TILES = 4 * ((1 << 24) - 8)
    fs = [rec.filt(4, m, d, dt) for m, d, dt in MIX]
    for ot in OUT_TYPES:
        ob = 4 if ot == F32 else 2
        for count in (2, 3, 4):
            rc, err, lines = record(rec, variant, fs[:count], OUTS[:count], ot, CH, L)
            assert rc == 0, err
            K = 2 if count == 4 else count
            per_launch = MAX_TILES // (1 + 2 * K)                          # one tile per channel, the edge items of every output counted
            groups = -(-CH // per_launch)
            assert len(lines) == groups * (2 if count == 4 else 1) and groups > 1
            for first in range(0, len(lines), groups):
                c0 = 0
                for line in lines[first:first + groups]:
                    head, outs = fields(line)
                    nc = int(head["total_tiles"])
                    assert int(head["k"]) == K and int(head["tiles_per_channel"]) == 1 and nc == min(per_launch, CH - c0)
                    assert int(head["edge_items"]) == (0 if variant == "valid" else 2 * K * nc)
                    assert int(head["grid"]) == ((nc + int(head["edge_items"]) + 3) // 4 + 7) // 8 * 8 < 1 << 24
                    assert int(head["in"], 16) == IN + c0 * L * 2
                    out_ld = L
                    assert {int(o["out"], 16) - c0 * out_ld * ob for o in outs[:K]} == set(OUTS[first // groups * 2:first // groups * 2 + K])
                    c0 += nc
                assert c0 == CH


def test_builds_without_the_launcher_refuse_counts_2_to_4(tmp_path):
    """sg_api_1d.cpp linked WITHOUT an object that defines sg1d_launch_multi_i16: the symbol is weak, the link closes under -z defs, and counts 2..4
    refuse with a text instead of calling through a null pointer.  With the single int16 launcher linked count 1 is still served; in the build of
    tests/test_launch_record_1d.py, which links neither int16 launcher, count 1 refuses as the single int16 call does there."""
    if not os.path.exists(HIP_HEADER):
        pytest.skip("hip/hip_runtime_api.h is not installed")
    from tests.test_launch_record_1d import build
    (tmp_path / "single").mkdir()
    R = Recorder(build_recorder(str(tmp_path / "single"), ("launch_i16_mock.cpp",)))
    fs = [R.filt(4, m, d, dt) for m, d, dt in MIX]
    for variant, name in zip(("full", "valid"), NAMES):
        for count in (2, 3, 4):
            for ot in OUT_TYPES:
                rc, err, lines = record(R, variant, fs[:count], OUTS[:count], ot)
                assert rc == -1 and "object not linked" in err and name in err and not lines
        # the argument checks still come first
        rc, err, lines = record(R, variant, fs[:2], [OUT0, IN], I16)
        assert rc == -1 and "d_outs[1] overlaps d_in" in err and not lines
        rc, err, lines = record(R, variant, fs[:1], OUTS[:1], I16)
        assert rc == 0 and len(lines) == 1 and lines[0].startswith("i16 n=4 moment_terms=0 ")
    lib = load(build(str(tmp_path)))
    for name in NAMES:
        getattr(lib, name).argtypes = ARGS
    R = Recorder(lib)
    fs = [R.filt(4, m, d, dt) for m, d, dt in MIX]
    for count in (1, 2, 3, 4):
        rc, err, lines = record(R, "full", fs[:count], OUTS[:count], I16)
        assert rc == -1 and "object not linked" in err and NAMES[0] in err and not lines
    rc, err, lines = record(R, "full", fs[:2], OUTS[:2], I16, ch=0)
    assert rc == 0 and not lines
