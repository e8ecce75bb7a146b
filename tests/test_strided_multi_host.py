"""savgol_apply_strided_multi_batch_f32 on a CPU: both symbols and their ctypes bindings, every refusal in the header's order (fake device addresses, no
device), the host rule, and what a fused call enqueues.

csrc/sg_k1d_strided_multi_host.hpp (strided_multi_plan) is built with plain g++ -Wall -Wextra -Werror into tests/mock/strided_multi_plan.cpp, which
prints one line per call; every line is held to the rule restated in tests/strided_multi_rule.py, and so is _route of the built library on the same
table.  csrc/sg_api_1d.cpp built against the launch recorder plus tests/mock/launch_strided_multi_mock.cpp records what a fused call enqueues: the
launches, the channel split, the edge items, and job k's fields against the single call's own job; the lines are pinned in
tests/golden/strided_multi_launch_record.txt (python tests/test_strided_multi_host.py --record rewrites it).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import strided_multi_rule as rule
from tests.test_launch_record_1d import CSRC, HIP_HEADER, ROCM, Recorder, SavgolFilter, load

NAME = "savgol_apply_strided_multi_batch_f32"
GOLDEN = os.path.join(ROOT, "tests", "golden", "strided_multi_launch_record.txt")
REF, CLE, AWARE = 1, 16, 32
IN, OUT = 0x100000000000, 0x200000000000             # fake device addresses: nothing touches them


# ---- the table of calls: (label, jobs [(n, boundary, in_offset, out_offset)], d_in, in_stride, in_pitch, d_out, out_stride, out_pitch, channels, count, flags)
def table():
    out = []

    def add(label, jobs, rec=16, ch=3, count=4000, d_in=IN, d_out=IN, flags=0, in_stride=None, out_stride=None, in_pitch=None, out_pitch=None, slack=0):
        in_stride = rec if in_stride is None else in_stride
        out_stride = rec if out_stride is None else out_stride
        in_pitch = (count + slack) * in_stride if in_pitch is None else in_pitch
        out_pitch = (count + slack) * out_stride if out_pitch is None else out_pitch
        out.append((label, [(n, b, i, o) for n, b, i, o in jobs], d_in, in_stride, in_pitch, d_out, out_stride, out_pitch, ch, count, flags))

    two = [(5, 0, 0, 8), (5, 0, 4, 12)]
    add("same records, fields 0,1 -> 2,3", two)
    add("same records, pitch with slack", two, slack=3)
    add("two arrays", two, d_out=OUT)
    add("two arrays, one channel, short", two, d_out=OUT, ch=1, count=11)
    # every alignment failure, one at a time
    add("input field address off by 2", [(5, 0, 2, 8), (5, 0, 4, 12)])
    add("output field address off by 2", [(5, 0, 0, 8), (5, 0, 4, 14)], d_out=OUT)
    add("input base off by 1", two, d_in=IN + 1, d_out=OUT)
    add("output base off by 2", two, d_out=OUT + 2)
    add("in_stride 18", two, d_out=OUT, in_stride=18)
    add("out_stride 18", two, d_out=OUT, out_stride=18)
    add("in_pitch off by 2", two, d_out=OUT, in_pitch=4000 * 16 + 2)
    add("out_pitch off by 2", two, d_out=OUT, out_pitch=4000 * 16 + 2)
    add("in_stride 0", two, d_out=OUT, in_stride=0, in_pitch=64)
    add("out_stride 0", two, d_out=OUT, out_stride=0, out_pitch=64)
    # record sizes: the measured ones are fused, others and unequal strides are not
    for rec in (8, 12, 16, 20, 24, 28, 32, 36, 64, 68, 128):
        if rec >= 12:                                                      # (an 8-byte record has no room for two outputs beside an input)
            add(f"same records of {rec} bytes", [(5, 0, 0, rec - 8), (5, 0, 4, rec - 4)] if rec >= 16 else [(5, 0, 0, 4), (5, 0, 0, 8)], rec=rec)
        add(f"two arrays of {rec}-byte records", [(5, 0, 0, 0), (5, 0, 4, 4)], rec=rec, d_out=OUT)
    add("8-byte records into 16-byte records", [(5, 0, 0, 0), (5, 0, 4, 4)], d_out=OUT, in_stride=8, out_stride=16)
    # shared bytes
    add("output equal to its own input field", [(5, 0, 0, 0), (5, 0, 4, 12)])
    add("output equal to another job's input field", [(5, 0, 0, 8), (5, 0, 8, 12)])
    add("read-after-write chain", [(5, 0, 0, 4), (5, 0, 4, 8), (5, 0, 8, 12)])
    add("write-after-read: a later job's output is an earlier job's input", [(5, 0, 0, 8), (5, 0, 4, 0)])
    add("two jobs, one output field", [(5, 0, 0, 8), (5, 0, 4, 8)])
    add("output 2 bytes into another output", [(5, 0, 0, 8), (5, 0, 4, 10)], rec=32)
    add("output 2 bytes into another output, two arrays", [(5, 0, 0, 8), (5, 0, 4, 10)], rec=32, d_out=OUT)
    add("output 2 bytes into an input field", [(5, 0, 0, 8), (5, 0, 4, 6)], rec=32)
    add("two grids that overlap with different strides", two, d_out=IN + 4, out_stride=32)
    add("two grids that overlap with different pitches", two, d_out=IN, out_pitch=4000 * 16 + 16)
    add("one grid whose pitch holds no whole number of records", [(5, 0, 0, 4), (5, 0, 0, 8)], rec=12, in_pitch=4000 * 12 + 4, out_pitch=4000 * 12 + 4)
    add("the output array right behind the input array", two, d_out=IN + 3 * 4000 * 16)
    add("the output array one record into the input array's end", two, d_out=IN + 3 * 4000 * 16 - 16)
    add("jobs share one input field", [(5, 0, 0, 4), (5, 0, 0, 8), (5, 0, 0, 12)])
    # filters and flags
    add("mixed half windows", [(5, 0, 0, 8), (6, 0, 4, 12)])
    add("mixed half windows, the last job", [(5, 0, 0, 4), (5, 0, 0, 8), (4, 0, 0, 12)])
    add("mixed boundary, default flags", [(5, 0, 0, 8), (5, 1, 4, 12)])
    add("mixed boundary, BOUNDARY_AWARE", [(5, 0, 0, 8), (5, 1, 4, 12)], flags=AWARE)
    add("equal boundary REFLECT, BOUNDARY_AWARE", [(5, 1, 0, 8), (5, 1, 4, 12)], flags=AWARE)
    add("REFERENCE_SUMMATION", two, flags=REF)
    add("REFERENCE_SUMMATION with BOUNDARY_AWARE", two, flags=REF | AWARE)
    add("CORRECT_LEADING_EDGE", two, flags=CLE)
    add("count beyond one launch", two, rec=8, ch=1, count=(1 << 30) + 1, d_out=OUT)
    add("count at the bound", [(5, 0, 0, 0), (5, 0, 4, 4)], rec=8, ch=1, count=1 << 30, d_out=OUT)
    # job counts: 64-byte records, field k -> field k of a second array
    for njobs in (1, 2, 3, 4, 5, 7, 8, 9, 10, 12, 13, 16):
        add(f"{njobs} jobs on 64-byte records", [(13, 0, 4 * k, 4 * k) for k in range(njobs)], rec=64, d_out=OUT)
        add(f"{njobs} jobs on 64-byte records, REFERENCE_SUMMATION", [(13, 0, 4 * k, 4 * k) for k in range(njobs)], rec=64, d_out=OUT, flags=REF)
    add("8 jobs inside 64-byte records", [(32, 0, 4 * k, 32 + 4 * k) for k in range(8)], rec=64)
    return out


def as_rule_call(row):
    label, jobs, d_in, in_stride, in_pitch, d_out, out_stride, out_pitch, ch, count, flags = row
    return ([(n, b, d_in + i, d_out + o) for n, b, i, o in jobs], in_stride, in_pitch, out_stride, out_pitch, ch, count, flags)


def test_symbols_exported_and_bound(sg):
    for name, args in ((NAME, 12), (NAME + "_route", 11)):
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == args
    assert callable(sg.apply_strided_multi_batch) and callable(sg.apply_strided_multi_batch_route)
    assert sg.SAVGOL_STRIDED_MULTI_MAX_JOBS == rule.MAX_JOBS == 16
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    assert NAME in names and NAME + "_route" in names
    assert not [line for line in out.splitlines() if "sg1d_launch_strided_multi" in line]       # nothing of the new objects leaks past the version script
    header = open(os.path.join(ROOT, "include", "savgol_hip.h")).read()
    assert "enum { SAVGOL_STRIDED_MULTI_MAX_JOBS = 16 };" in header
    assert C.sizeof(sg.SavgolFieldJob) == 3 * C.sizeof(C.c_size_t)


def test_refusals_in_the_headers_order_need_no_device(sg):
    """every refusal, then pairs of faults: the one that comes first in the documented order is reported; both entry points, the same text"""
    L = sg.lib()
    a, b = sg.Filter(5, 2, 0), sg.Filter(6, 3, 1)
    bad = sg.Filter(5, 3, 1)
    bad.ptr.contents.window_size = 13
    J = sg.SavgolFieldJob
    FP = C.POINTER(sg.SavgolFilter)

    def jobs(*fs):
        return (J * max(len(fs), 1))(*[J(f.ptr if f is not None else FP(), 4 * k, 8 + 4 * k) for k, f in enumerate(fs)])

    good = dict(jobs=jobs(a, a), njobs=2, d_in=IN, d_out=IN, count=1000, channels=3, flags=0)
    cases = [
        (dict(flags=0x1000), "bad flags 0x1000"),                                                   # 1
        (dict(flags=4 | 8), "bad flags 0xc"),
        (dict(jobs=None), "NULL pointer"),                                                           # 2
        (dict(d_in=None), "NULL pointer"),
        (dict(d_out=None), "NULL pointer"),
        (dict(njobs=0), "njobs 0 outside 1..16"),                                                   # 3
        (dict(njobs=-1), "njobs -1 outside 1..16"),
        (dict(jobs=jobs(*[a] * 17), njobs=17), "njobs 17 outside 1..16"),
        (dict(jobs=jobs(a, None)), "NULL pointer (jobs[1].filter)"),                                # 4
        (dict(jobs=jobs(a, bad)), "not a valid SavgolFilter"),                                      # 5
        (dict(count=10), "count < window size (jobs[0])"),                                           # 6
        (dict(jobs=jobs(a, b), count=12), "count < window size (jobs[1])"),
        # two faults: the first in order wins
        (dict(flags=0x1000, jobs=None), "bad flags 0x1000"),                                         # 1 before 2
        (dict(d_in=None, njobs=0), "NULL pointer"),                                                  # 2 before 3
        (dict(jobs=jobs(a, None), njobs=17), "njobs 17 outside 1..16"),                              # 3 before 4
        (dict(jobs=jobs(bad, None)), "NULL pointer (jobs[1].filter)"),                               # 4 before 5
        (dict(jobs=jobs(a, bad), count=10), "not a valid SavgolFilter"),                             # 5 before 6
        (dict(count=10, channels=0), "count < window size (jobs[0])"),                               # 6 before the empty batch
    ]
    for kw, text in cases:
        k = dict(good, **kw)
        head = (k["jobs"], k["njobs"], k["d_in"], 16, k["count"] * 16, k["d_out"], 16, k["count"] * 16, k["channels"], k["count"], k["flags"])
        for fn, tail in ((L.savgol_apply_strided_multi_batch_f32, (None,)), (L.savgol_apply_strided_multi_batch_f32_route, ())):
            assert fn(*head, *tail) == -1, text
            err = sg.last_error()
            assert err.startswith(NAME + ":") and text in err, (text, err)
    # channels == 0: the checks pass, nothing to do
    head = (good["jobs"], 2, IN, 16, 16000, IN, 16, 16000, 0, 1000, 0)
    assert L.savgol_apply_strided_multi_batch_f32(*head, None) == 0
    assert L.savgol_apply_strided_multi_batch_f32_route(*head) == 0
    with pytest.raises(RuntimeError):
        sg.apply_strided_multi_batch([(a, 0, 8), (a, 4, 12)], IN, 16, 16000, IN, 16, 16000, 3, 10)


def test_no_cpu_fallback_without_device(sg):
    """with valid arguments and no GPU the call must FAIL on both routes, not compute on the host; _route needs no device"""
    if sg.device_count() > 0:
        pytest.skip("a GPU is present")
    a = sg.Filter(5, 2, 0)
    for jobs, want in (([(a, 0, 8), (a, 4, 12)], 1), ([(a, 0, 4), (a, 4, 8)], 0)):
        assert sg.apply_strided_multi_batch_route(jobs, IN, 16, 16000, IN, 16, 16000, 3, 1000) == want
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            sg.apply_strided_multi_batch(jobs, IN, 16, 16000, IN, 16, 16000, 3, 1000)


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("strided_multi_plan"))
    exe = os.path.join(tmp, "strided_multi_plan")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mock", "strided_multi_plan.cpp")],
                   check=True)
    text = ""
    for row in table():
        jobs, in_stride, in_pitch, out_stride, out_pitch, ch, count, flags = as_rule_call(row)
        text += f"{len(jobs)} {in_stride} {in_pitch} {out_stride} {out_pitch} {ch} {count} {int(bool(flags & AWARE))} {int(bool(flags & REF))}\n"
        text += "".join(f"{n} {b} {i} {o}\n" for n, b, i, o in jobs)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[-1] == f"bounds jobs={rule.MAX_JOBS} per_launch=4 max_length={rule.MAX_LENGTH}"
    return out[:-1]


def test_the_host_rule_is_the_restated_rule(plan_lines):
    rows = table()
    assert len(plan_lines) == len(rows)
    seen = set()
    for row, line in zip(rows, plan_lines):
        groups = rule.groups(*as_rule_call(row))
        want = f"launches={sum(1 for g in groups if g >= 2)} groups={','.join(map(str, groups))}"
        assert line == want, (row[0], line, want)
        seen.add(rule.launches(*as_rule_call(row)))
    # the table takes both routes and every launch count 16 jobs can make
    assert seen == {0, 1, 2, 3, 4}
    by_label = {row[0]: rule.groups(*as_rule_call(row)) for row in rows}
    assert by_label["same records, fields 0,1 -> 2,3"] == [2] and by_label["two arrays"] == [2]
    assert by_label["5 jobs on 64-byte records"] == [4, 1] and by_label["7 jobs on 64-byte records"] == [4, 3] and by_label["16 jobs on 64-byte records"] == [4] * 4
    assert by_label["1 jobs on 64-byte records"] == [] and by_label["read-after-write chain"] == [] and by_label["mixed boundary, BOUNDARY_AWARE"] == []
    assert by_label["mixed boundary, default flags"] == [2] and by_label["jobs share one input field"] == [3]
    for rec in (8, 12, 16, 20, 32, 64):
        assert by_label[f"two arrays of {rec}-byte records"] == [2] and (rec == 8 or by_label[f"same records of {rec} bytes"] == [2])
    for rec in (24, 28, 36, 68, 128):
        assert by_label[f"same records of {rec} bytes"] == [] and by_label[f"two arrays of {rec}-byte records"] == []


def test_route_of_the_library_agrees_with_the_rule(sg):
    L = sg.lib()
    filters = {}
    for row in table():
        label, jobs, d_in, in_stride, in_pitch, d_out, out_stride, out_pitch, ch, count, flags = row
        for n, b, _, _ in jobs:
            if (n, b) not in filters:
                filters[(n, b)] = sg.Filter(n, 2, 0, 1.0, b)
        arr = (sg.SavgolFieldJob * len(jobs))(*[sg.SavgolFieldJob(filters[(n, b)].ptr, i, o) for n, b, i, o in jobs])
        got = L.savgol_apply_strided_multi_batch_f32_route(arr, len(jobs), d_in, in_stride, in_pitch, d_out, out_stride, out_pitch, ch, count, flags)
        assert got == rule.launches(*as_rule_call(row)), (label, got, sg.last_error())


# ---- what a fused call enqueues: csrc/sg_api_1d.cpp against the launch recorder + the mock of the new launcher --------------------------------------
STREAM = 0x5700


def build_recorder(tmp):
    so = os.path.join(tmp, "libsg_launch_recorder_strided_multi.so")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]
    wobj = os.path.join(tmp, "sg_weights.o")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", *inc, "-c", os.path.join(CSRC, "sg_weights.c"), "-o", wobj], check=True)
    # -Bsymbolic: the recorder's own hipGetLastError & co. are the ones its code calls, whatever HIP runtime an earlier test has made global in this process
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wl,-z,defs", "-Wl,-Bsymbolic", *inc, "-o", so, os.path.join(CSRC, "sg_api_1d.cpp"),
                    os.path.join(CSRC, "sg_k1d_moment_fit.cpp"), os.path.join(ROOT, "tests", "mock", "launch_recorder_1d.cpp"),
                    os.path.join(ROOT, "tests", "mock", "launch_strided_multi_mock.cpp"), wobj, "-lm", "-lpthread"], check=True)
    return bind(load(so))


def bind(lib):
    P, Z, U, I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    lib.savgol_apply_strided_multi_batch_f32.argtypes = [P, I, P, Z, Z, P, Z, Z, Z, Z, U, P]
    lib.savgol_apply_strided_multi_batch_f32_route.argtypes = [P, I, P, Z, Z, P, Z, Z, Z, Z, U]
    return lib


class FieldJob(C.Structure):
    _fields_ = [("filter", C.POINTER(SavgolFilter)), ("in_offset", C.c_size_t), ("out_offset", C.c_size_t)]


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    if not os.path.exists(HIP_HEADER):
        pytest.skip("hip/hip_runtime_api.h is not installed")
    return Recorder(build_recorder(str(tmp_path_factory.mktemp("launch_recorder_strided_multi"))))


def record(R, jobs, rec_bytes=16, ch=3, count=4000, d_out=IN, flags=0):
    """one multi call on a fresh record -> (rc, error text, the record's launcher lines)"""
    arr = (FieldJob * len(jobs))(*[FieldJob(f, i, o) for f, i, o in jobs])
    R.begin()
    rc = R.call(NAME, arr, len(jobs), IN, rec_bytes, count * rec_bytes, d_out, rec_bytes, count * rec_bytes, ch, count, flags, STREAM)
    log, _ = R.end()
    return rc, R.lib.savgol_hip_last_error().decode(), [l for l in log.splitlines() if l and not l.startswith(("call ", "-> ", "part "))]


def record_single(R, f, i, o, rec_bytes=16, ch=3, count=4000, d_out=IN, flags=0):
    R.begin()
    rc = R.call("savgol_apply_strided_batch_f32_ex", f, IN, rec_bytes, i, count * rec_bytes, d_out, rec_bytes, o, count * rec_bytes, ch, count, flags, STREAM)
    log, _ = R.end()
    assert rc == 0, R.lib.savgol_hip_last_error().decode()
    return [l for l in log.splitlines() if l and not l.startswith(("call ", "-> ", "part "))]


def fields(line):
    """'name k=v ... [0]{k=v ...} ...' -> ({k: v} of the part before the jobs, [{k: v}] per job)"""
    head, *jobs = re.split(r" \[\d\]\{", line)
    kv = lambda text: dict(re.findall(r"(\w+)=([^\s{}]+)", text))
    return kv(head), [kv(j) for j in jobs]


MIX = ((2, 0, 1.0), (3, 1, 0.5), (4, 2, 0.5), (4, 0, 1.0), (3, 1, 1.0), (2, 0, 1.0), (4, 2, 1.0))      # (poly_order, derivative, time_step) of jobs 0..6
GRID = ("in_pitch", "out_pitch", "in_stride", "out_stride", "length", "tiles_per_channel", "total_tiles", "tpc_magic", "tpc_shift", "store_lo", "store_hi")


@pytest.mark.parametrize("flags,mode", ((0, 0), (0, 1), (CLE, 0), (AWARE, 0), (AWARE, 1), (AWARE | CLE, 3), (AWARE, 300)))
@pytest.mark.parametrize("n", (1, 14, 15, 23, 32))
def test_a_fused_calls_jobs_are_the_single_calls_jobs(rec, n, flags, mode):
    """2, 3, 4 jobs: one launch; 5: a launch of four and a single call; 7: launches of four and three.  Job k of a launch carries the single call's
    taps, dt_inv, flags and edge rows, the grid the single call's geometry, the field addresses split into grid base + offset"""
    fs = [rec.filt(n, m, d, dt, mode) for m, d, dt in MIX if m < 2 * n + 1]
    fs = (fs * 7)[:7]
    for njobs, want in ((2, ["strided_multi"]), (3, ["strided_multi"]), (4, ["strided_multi"]), (5, ["strided_multi", "strided"]), (7, ["strided_multi"] * 2)):
        for ch, count, d_out in ((3, 4000, IN), (2, 2 * n + 1, OUT), (5, 9004, OUT)):
            jobs = [(fs[k], 4 * k, 32 + 4 * k) for k in range(njobs)]
            rc, err, lines = record(rec, jobs, 64, ch, count, d_out, flags)
            assert rc == 0, err
            assert [l.split(" ", 1)[0].split("_f32_")[0] for l in lines] == want, lines
            k0 = 0
            for line in lines:
                if line.startswith("strided_f32_"):
                    assert line == record_single(rec, *jobs[k0], 64, ch, count, d_out, flags)[0]
                    k0 += 1
                    continue
                head, per = fields(line)
                nj = int(head["njobs"])
                assert nj == min(4, njobs - k0) and int(head["n"]) == n and head["stream"] == hex(STREAM)
                assert int(head["in"], 16) == IN and int(head["out"], 16) == d_out
                items = int(head["total_tiles"]) + int(head["edge_items"])
                assert int(head["grid"]) == (items + 7) // 8 * 8
                for k in range(nj):
                    single = record_single(rec, *jobs[k0 + k], 64, ch, count, d_out, flags)
                    assert len(single) == 1
                    job = dict(re.findall(r"(\w+)=([^\s{}]+)", single[0]))
                    assert {key: head[key] for key in GRID} == {key: job[key] for key in GRID}, (line, single)
                    assert int(head["edge_items"]) == nj * int(job["edge_items"])
                    assert (per[k]["dt_inv"], per[k]["flags"], per[k]["taps"]) == (job["dt_inv"], job["flags"], job["taps"]), (k, line, single)
                    assert (per[k]["has_edges"] == "1") == (job["edges"] != "null")
                    assert (int(per[k]["in_off"]), int(per[k]["out_off"])) == (jobs[k0 + k][1], jobs[k0 + k][2])
                    assert int(head["flags"], 16) == int(job["flags"], 16) & 0xff
                for k in range(nj, 4):                                      # the unused slots are zero
                    assert {key: per[k][key] for key in ("in_off", "out_off", "has_edges", "dt_inv", "flags")} == dict(in_off="0", out_off="0", has_edges="0", dt_inv="0x0p+0", flags="0x0")
                k0 += nj
            assert k0 == njobs


def test_a_call_that_falls_back_is_the_single_calls_in_order(rec):
    a, b = rec.filt(5, 2, 0), rec.filt(5, 3, 1, 0.5)
    for jobs, flags in (([(a, 0, 4), (b, 4, 8)], 0), ([(a, 0, 8), (b, 4, 12)], REF), ([(a, 2, 8), (b, 4, 12)], 0), ([(a, 0, 8), (rec.filt(6, 2, 0), 4, 12)], AWARE)):
        rc, err, lines = record(rec, jobs, flags=flags)
        assert rc == 0, err
        rec.begin()                                                        # the single calls on ONE record: its scratch allocations are numbered
        for f, i, o in jobs:
            assert rec.call("savgol_apply_strided_batch_f32_ex", f, IN, 16, i, 4000 * 16, IN, 16, o, 4000 * 16, 3, 4000, flags, STREAM) == 0
        want = [l for l in rec.end()[0].splitlines() if l and not l.startswith(("call ", "-> ", "part "))]
        assert lines == want and not any(l.startswith("strided_multi") for l in lines)


def test_30_million_short_channels_split_over_channels(rec):
    CH, count = 30000000, 100
    MAX_TILES = 4 * ((1 << 24) - 8)
    fs = [rec.filt(4, m, d, dt) for m, d, dt in MIX]
    for njobs in (2, 3, 4):
        rc, err, lines = record(rec, [(fs[k], 4 * k, 4 * k) for k in range(njobs)], 16, CH, count, OUT)
        assert rc == 0, err
        per_launch = MAX_TILES // (1 + 2 * njobs)                          # one tile per channel, the edge items of every job counted
        assert len(lines) == -(-CH // per_launch) > 1
        c0 = 0
        for line in lines:
            head, _ = fields(line)
            nc = int(head["total_tiles"])
            assert nc == min(per_launch, CH - c0) and int(head["edge_items"]) == 2 * njobs * nc
            assert int(head["grid"]) == (nc + 2 * njobs * nc + 7) // 8 * 8 <= 1 << 26 and int(head["grid"]) * 64 < 1 << 32
            assert int(head["in"], 16) == IN + c0 * count * 16 and int(head["out"], 16) == OUT + c0 * count * 16
            c0 += nc
        assert c0 == CH


def test_the_existing_record_build_refuses_without_the_launcher(tmp_path):
    """sg_api_1d.cpp linked WITHOUT an object that defines the launcher (the build of tests/test_launch_record_1d.py): the symbol is weak, the link
    closes under -z defs, and a fused call refuses with a text instead of calling through a null pointer; _route needs no launcher"""
    if not os.path.exists(HIP_HEADER):
        pytest.skip("hip/hip_runtime_api.h is not installed")
    from tests.test_launch_record_1d import build
    R = Recorder(bind(load(build(str(tmp_path)))))
    a = R.filt(4, 2, 0)
    rc, err, lines = record(R, [(a, 0, 8), (a, 4, 12)])
    assert rc == -1 and "object not linked" in err and NAME in err and not lines
    arr = (FieldJob * 2)(FieldJob(a, 0, 8), FieldJob(a, 4, 12))
    assert R.lib.savgol_apply_strided_multi_batch_f32_route(arr, 2, IN, 16, 64000, IN, 16, 64000, 3, 4000, 0) == 1


# ---- the pinned record -----------------------------------------------------------------------------------------------------------------------------
def golden_cases(R):
    """[(id, launcher lines)]: a few fused calls whose every kernel argument is pinned"""
    out = []
    for n, mode, flags in ((1, 0, 0), (5, 0, 0), (5, 1, AWARE), (13, 0, CLE), (32, 2, AWARE | CLE), (32, 0, 0)):
        fs = [R.filt(n, m, d, dt, mode) for m, d, dt in MIX if m < 2 * n + 1]
        fs = (fs * 7)[:7]
        for njobs, rec_bytes, ch, count, d_out in ((2, 8, 3, 4000, OUT), (3, 16, 2, 2 * n + 1, IN), (4, 32, 4, 5000, IN), (5, 64, 1, 70001, OUT), (7, 64, 3, 2048 + 2 * n + 3, IN)):
            half = rec_bytes // 2 if d_out == IN else 0
            jobs = [(fs[k], (4 * k) % max(half, 4) if d_out == IN else 4 * k % rec_bytes, half + 4 * k if d_out == IN else 4 * k % rec_bytes) for k in range(njobs)]
            if d_out == IN and njobs * 4 > half:
                jobs = [(fs[k], 0, 4 * (k + 1)) for k in range(njobs)]                   # one input field into the others
            rc, err, lines = record(R, jobs, rec_bytes, ch, count, d_out, flags)
            assert rc == 0 and any(l.startswith("strided_multi") for l in lines), (err, lines)
            out.append((f"n{n}/mode{mode}/flags{flags:#x}/jobs{njobs}/rec{rec_bytes}/{ch}x{count}/{'same' if d_out == IN else 'two'}", lines))
    return out


def golden_text(R):
    return "".join(f"{cid}\t{k}\t{line}\n" for cid, lines in golden_cases(R) for k, line in enumerate(lines))


def test_launch_record_matches_golden(rec):
    got = golden_text(rec).splitlines()
    want = open(GOLDEN).read().splitlines()
    assert len(got) == len(want) > 30
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} lines differ from tests/golden/strided_multi_launch_record.txt, the first:\n now:    {bad[0][0]}\n golden: {bad[0][1]}"


if __name__ == "__main__":
    if "--record" in sys.argv:
        with tempfile.TemporaryDirectory() as tmp:
            text = golden_text(Recorder(build_recorder(tmp)))
        with open(GOLDEN, "w") as fh:
            fh.write(text)
        print(f"wrote {len(text.splitlines())} lines to {GOLDEN}")
