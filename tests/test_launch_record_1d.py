"""What the host side of the 1-D path ENQUEUES, recorded on a CPU: csrc/sg_api_1d.cpp (with sg_weights.c and sg_k1d_moment_fit.cpp) is built with
g++ against tests/mock/launch_recorder_1d.cpp, which defines every launcher, sg:: runtime function and HIP call the file leaves undefined and writes
one line per call -- name, scalars, the job struct field by field, tap digests, pointers as names.  The public C entry points are driven through
ctypes over a case matrix that puts every branch of the dispatcher on record (tile choice, block moments, channel splits, in place, channels beyond
2^30 samples, reference order, multi-output, 16-bit storage, strided, the host-pointer ladder, every refusal), and every case's return codes, error
texts and record are compared with tests/golden/launch_record_1d.txt: one line per case (the ~3000 parts of the matrix that share a route and a
half window are one case) -- id, number of parts, return codes, the launcher sequence in short form, sha256 of the full record.  A host-side change that alters one kernel argument of one launch shows up here, without a GPU.

    python tests/test_launch_record_1d.py --record        rewrites the golden from the tree's sources
    python tests/test_launch_record_1d.py --dump DIR      writes every case's full record to DIR/<n>.txt + index (to diff two trees)

No GPU needed; skips only where the HIP runtime API header is absent."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "savitzky-golay-filter_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_record_1d.txt")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIP_HEADER = os.path.join(ROCM, "include", "hip", "hip_runtime_api.h")

REF, PLAIN, NARROW, WIDE, CLE, AWARE, M64 = 1, 2, 4, 8, 16, 32, 64
FLAGS7 = (0, PLAIN, REF, NARROW, WIDE, CLE, M64)
OPT_CLE, OPT_REF, OPT_PLAIN, OPT_AWARE, OPT_TILE = 1, 2, 3, 4, 5
F32, F16, BF16 = 0, 1, 2
# every edge of wide_vectors_per_lane, MOMENTH_MIN_N, MOMENT_MIN_N and the four kernel-object groups
HALF_WINDOWS = (1, 4, 12, 13, 18, 19, 20, 23, 24, 28, 32)
POLY_DERIV = ((0, 0), (2, 0), (3, 1), (4, 2), (4, 0))
# fake device addresses (names in the record: "in+off", "out+off", ...), 1 TiB each
SPAN = 1 << 40
IN, OUT, OUT1, OUT2, OUT3 = 0x100000000000, 0x200000000000, 0x210000000000, 0x220000000000, 0x230000000000
BASES = (("in", IN), ("out", OUT), ("out1", OUT1), ("out2", OUT2), ("out3", OUT3))
STREAM = 0x5700


class SavgolConfig(C.Structure):
    _fields_ = [("half_window", C.c_uint8), ("poly_order", C.c_uint8), ("derivative", C.c_uint8), ("time_step", C.c_float), ("boundary", C.c_int)]


class SavgolFilter(C.Structure):
    _fields_ = [("config", SavgolConfig), ("window_size", C.c_int), ("dt_scale", C.c_float), ("center_weights", C.c_float * 65),
                ("edge_weights", (C.c_float * 65) * 32)]


def build(tmp):
    so = os.path.join(tmp, "libsg_launch_recorder_1d.so")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]
    wobj = os.path.join(tmp, "sg_weights.o")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", *inc, "-c", os.path.join(CSRC, "sg_weights.c"), "-o", wobj], check=True)
    # -z defs: the list of symbols the recorder has to define is closed; a new undefined one fails the link, not the load
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wl,-z,defs", *inc, "-o", so, os.path.join(CSRC, "sg_api_1d.cpp"),
                    os.path.join(CSRC, "sg_k1d_moment_fit.cpp"), os.path.join(ROOT, "tests", "mock", "launch_recorder_1d.cpp"), wobj, "-lm", "-lpthread"],
                   check=True)
    return so


def load(so):
    lib = C.CDLL(so)
    P, Z, U, I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    lib.savgol_create.restype = C.POINTER(SavgolFilter)
    lib.savgol_create.argtypes = [C.POINTER(SavgolConfig)]
    lib.savgol_hip_last_error.restype = C.c_char_p
    lib.rec_log.restype = C.c_char_p
    lib.rec_add_base.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t]
    lib.rec_note.argtypes = [C.c_char_p]
    batch = [P, P, P, Z, Z, Z, Z]
    for t in ("f32", "f64"):
        for v in ("", "_valid"):
            getattr(lib, f"savgol_apply{v}_batch_{t}").argtypes = batch + [P]
            getattr(lib, f"savgol_apply{v}_batch_{t}_ex").argtypes = batch + [U, P]
    for v in ("", "_valid"):
        getattr(lib, f"savgol_apply{v}_batch_f64_tol").argtypes = batch + [C.c_double, P]
        getattr(lib, f"savgol_apply{v}_multi_batch_f32").argtypes = [P, I, P, P, Z, Z, Z, Z, U, P]
        getattr(lib, f"savgol_apply{v}_batch_h16").argtypes = [P, P, I, P, I, Z, Z, Z, Z, U, P]
    lib.savgol_apply_strided_batch_f32.argtypes = [P, P, Z, Z, Z, P, Z, Z, Z, Z, Z, P]
    lib.savgol_apply_strided_batch_f32_ex.argtypes = [P, P, Z, Z, Z, P, Z, Z, Z, Z, Z, U, P]
    lib.savgol_apply.argtypes = [P, P, P, Z]
    lib.savgol_apply_valid.argtypes = [P, P, Z, P]
    lib.savgol_apply_valid.restype = Z
    lib.savgol_apply_strided.argtypes = [P, P, Z, Z, P, Z, Z, Z]
    return lib


class Recorder:
    """one case = rec_reset, a few public calls (each noted in the record with its return code and error text), the record"""

    def __init__(self, lib):
        self.lib = lib
        self.filters = {}
        self.rcs = []

    def filt(self, n, m, d, dt=1.0, boundary=0):
        """a filter savgol_create built; `boundary` is written afterwards so that values the enum does not name get through"""
        key = (n, m, d, dt, boundary)
        if key not in self.filters:
            f = self.lib.savgol_create(C.byref(SavgolConfig(n, m, d, dt, 0)))
            assert f, key
            f.contents.config.boundary = boundary
            self.filters[key] = f
        return self.filters[key]

    def begin(self):
        self.lib.rec_reset()
        self.lib.rec_set_small(0)
        self.rcs = []
        self.bases()

    def bases(self, extra_bases=()):
        """the address ranges the record names: the fake device buffers, and a part's own host buffers"""
        self.lib.rec_clear_bases()
        for name, addr in BASES:
            self.lib.rec_add_base(name.encode(), addr, SPAN)
        self.lib.rec_add_base(b"below_in", IN - (1 << 32), 1 << 32)
        for name, addr, size in extra_bases:
            self.lib.rec_add_base(name.encode(), addr, size)

    def call(self, name, *args, note=""):
        self.lib.rec_clear_error()
        self.lib.rec_note(f"call {name} {note}".encode())
        rc = getattr(self.lib, name)(*args)
        self.lib.rec_note(f"-> rc={rc} err={self.lib.savgol_hip_last_error().decode()}".encode())
        self.rcs.append(int(rc))
        return rc

    def option(self, option, value):
        assert self.lib.savgol_hip_set_option(option, value) == 0

    def end(self):
        return self.lib.rec_log().decode(), list(self.rcs)


def valid_config(n, m, d):
    return m < 2 * n + 1 and d <= m


def configs(n, poly_deriv=POLY_DERIV):
    for m, d in poly_deriv:
        if valid_config(n, m, d):
            for dt in ((1.0, 0.5) if d else (1.0,)):           # dt_scale = dt^d: the time step only shows on derivatives
                yield m, d, dt


def cases():
    """[(id, fn(R))]: fn drives the calls of one part; the parts whose ids share their first three components make one case (one golden line)"""
    out = []

    def add(cid, fn):
        out.append((cid, fn))

    def batch_name(t, variant, ex=True):
        return f"savgol_apply{'_valid' if variant == 'valid' else ''}_batch_{t}" + ("_ex" if ex else "")

    def batch(R, t, variant, f, ch, L, flags, d_in=IN, d_out=OUT, in_ld=None, out_ld=None, stream=STREAM):
        R.call(batch_name(t, variant), f, d_in, d_out, ch, L, L if in_ld is None else in_ld, L if out_ld is None else out_ld, flags, stream,
               note=f"ch={ch} L={L} in_ld={in_ld} out_ld={out_ld} flags={flags:#x} d_in={d_in and d_in - IN} d_out={d_out and d_out - IN}")

    # ---- A. job setup: every filter x boundary mode x FULL / VALID, each case sweeping the seven flag words --------------------------------
    for t in ("f32", "f64"):
        for n in HALF_WINDOWS:
            for m, d, dt in configs(n):
                for variant, mode in (("full", 0), ("full", 1), ("full", 2), ("full", 3), ("valid", 0)):
                    def fn(R, t=t, n=n, m=m, d=d, dt=dt, variant=variant, mode=mode):
                        for flags in FLAGS7:
                            batch(R, t, variant, R.filt(n, m, d, dt, mode), 4, 1000, flags)
                    add(f"A/{t}/n{n}/m{m}d{d}dt{dt}/{variant}/mode{mode}/flags", fn)
            # a boundary value the enum does not name: zero padding (mode byte 255 beyond a byte, the value itself below)
            for m, d, dt in configs(n, ((2, 0), (3, 1))):
                for mode in (7, 300, -1):
                    def fn(R, t=t, n=n, m=m, d=d, dt=dt, mode=mode):
                        for flags in (0, REF, NARROW):
                            batch(R, t, "full", R.filt(n, m, d, dt, mode), 4, 1000, flags)
                        batch(R, t, "valid", R.filt(n, m, d, dt, mode), 4, 1000, 0)
                    add(f"A/{t}/n{n}/m{m}d{d}dt{dt}/unknown-mode{mode}", fn)

    # ---- B. shapes: tile choice by size, pitches, alignment, channel splits -----------------------------------------------------------------
    shapes = (("1x4096", dict(ch=1, L=4096)),
              ("3x70000-odd-pitch", dict(ch=3, L=70000, in_ld=70001, out_ld=70003)),
              ("3x70000-off-16", dict(ch=3, L=70000, in_ld=70004, out_ld=70008, d_in=IN + 4, d_out=OUT + 8)),
              ("4096x2^20", dict(ch=4096, L=1 << 20)),
              ("16383x1000", dict(ch=16383, L=1000)),              # one tile per channel at any width: just below WIDE_TILE_MIN_TILES ...
              ("16384x1000", dict(ch=16384, L=1000)),              # ... and at it
              ("8191x3000", dict(ch=8191, L=3000)),
              ("8192x3000", dict(ch=8192, L=3000)),
              ("30000000x100", dict(ch=30000000, L=100)))          # split over channels below MAX_TILES_PER_LAUNCH
    for t in ("f32", "f64"):
        for n in (4, 12, 13, 18, 19, 24, 25, 32):
            for m, d, dt in ((2, 0, 1.0), (3, 1, 0.5)):
                for variant, mode in (("full", 0), ("full", 1), ("valid", 0)):
                    for sname, kw in shapes:
                        def fn(R, t=t, n=n, m=m, d=d, dt=dt, variant=variant, mode=mode, kw=kw):
                            for flags in (0, M64) if t == "f64" else (0, PLAIN):
                                batch(R, t, variant, R.filt(n, m, d, dt, mode), flags=flags, **kw)
                        add(f"B/{t}/n{n}/m{m}d{d}/{variant}/mode{mode}/{sname}", fn)

    # ---- channels longer than one launch indexes (enqueue_long) --------------------------------------------------------------------------------
    LONG = (1 << 30) + 1000
    for t in ("f32", "f64"):
        for n in (4, 32):
            for m, d, dt in ((2, 0, 1.0), (3, 1, 0.5)):
                for variant, mode in (("full", 0), ("full", 1), ("full", 2), ("full", 3), ("valid", 0)):
                    def fn(R, t=t, n=n, m=m, d=d, dt=dt, variant=variant, mode=mode):
                        for flags in (0, REF, PLAIN, CLE):
                            batch(R, t, variant, R.filt(n, m, d, dt, mode), 2, LONG, flags, in_ld=LONG + 24, out_ld=LONG + 8)
                    add(f"long/{t}/n{n}/m{m}d{d}/{variant}/mode{mode}", fn)
        def fn(R, t=t):
            f = R.filt(4, 2, 0)
            batch(R, t, "full", f, 2, LONG, 0, d_out=IN)                                  # in place is not served at this length
            batch(R, t, "full", f, 2, LONG, 0, d_out=IN + 4096)
            batch(R, t, "full", f, 2, LONG, 0, in_ld=LONG - 1)
            batch(R, t, "valid", f, 2, LONG, 0, out_ld=LONG - 9)
            batch(R, t, "valid", f, 2, LONG, 0, out_ld=LONG - 8)
            batch(R, t, "full", f, 0, LONG, 0)
            batch(R, t, "full", f, 1, 3 * (1 << 29) + 4, 0)                               # three whole segments and a remainder
        add(f"long/{t}/refusals-and-segments", fn)

    # ---- C. reference order: below and above the 2^16-sample switch to the packed kernel -------------------------------------------------------
    for n in (4, 32):
        for m, d, dt in ((2, 0, 1.0), (3, 1, 0.5)):
            for variant, mode in (("full", 0), ("full", 1), ("full", 2), ("valid", 0)):
                def fn(R, n=n, m=m, d=d, dt=dt, variant=variant, mode=mode):
                    f = R.filt(n, m, d, dt, mode)
                    for ch, L in ((1, 65535), (1, 65536), (4, 16383), (4, 16384), (4, 70000), (2000, 100), (700, 4 * (2 * n + 1) - 1), (700, 4 * (2 * n + 1))):
                        for flags in (REF, REF | CLE):
                            batch(R, "f32", variant, f, ch, L, flags)
                add(f"C/ref/n{n}/m{m}d{d}/{variant}/mode{mode}", fn)

    # ---- D. in place: odd and even tile counts, stash groups, the edge-row launches ------------------------------------------------------------
    inplace_shapes = (("4x1000", dict(ch=4, L=1000)), ("4x6144", dict(ch=4, L=6144)), ("4x8192", dict(ch=4, L=8192)), ("4x6145", dict(ch=4, L=6145)),
                      ("4x5000-pitch", dict(ch=4, L=5000, in_ld=5008, out_ld=5008)), ("100000x70000", dict(ch=100000, L=70000)),
                      ("5000000x100", dict(ch=5000000, L=100)), ("4096x2^20", dict(ch=4096, L=1 << 20)))
    for t in ("f32", "f64"):
        for n in (4, 13, 32):
            for m, d, dt in ((2, 0, 1.0), (3, 1, 0.5)):
                for mode in (0, 1, 2):
                    for sname, kw in inplace_shapes:
                        def fn(R, t=t, n=n, m=m, d=d, dt=dt, mode=mode, kw=kw):
                            for flags in (0, REF, NARROW, WIDE, CLE, M64):
                                batch(R, t, "full", R.filt(n, m, d, dt, mode), flags=flags, d_out=kw.get("d_in", IN), **kw)
                        add(f"D/{t}/n{n}/m{m}d{d}/mode{mode}/{sname}", fn)

    # ---- E. refusals of the batch calls ---------------------------------------------------------------------------------------------------------
    for t in ("f32", "f64"):
        for variant in ("full", "valid"):
            def fn(R, t=t, variant=variant):
                f = R.filt(5, 2, 0)
                elem = 4 if t == "f32" else 8
                batch(R, t, variant, None, 4, 1000, 0)
                batch(R, t, variant, f, 4, 1000, 0, d_in=None)
                batch(R, t, variant, f, 4, 1000, 0, d_out=None)
                batch(R, t, variant, f, 4, 10, 0)
                batch(R, t, variant, f, 4, 11, 0)                                          # the shortest row that is served
                batch(R, t, variant, f, 4, 1000, 0, in_ld=999)
                batch(R, t, variant, f, 4, 1000, 0, out_ld=989)
                batch(R, t, variant, f, 4, 1000, 0, out_ld=990)                            # VALID's row is 2n shorter
                batch(R, t, variant, f, 0, 1000, 0)
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN)                              # in place (VALID: a shifted overlap)
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN + elem)
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN + 4 * 1000 * elem - elem)
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN - 4 * 1000 * elem + elem)
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN, in_ld=1000, out_ld=1008)     # same base, another pitch: not "in place"
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN + 1000 * elem, in_ld=2000, out_ld=2000)      # interleaved rows: no overlap
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN + 999 * elem, in_ld=2000, out_ld=2000)       # interleaved, one element shared
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN - 1000 * elem, in_ld=2000, out_ld=2000)      # the output rows in front
                batch(R, t, variant, f, 4, 1000, 0, d_out=IN - 1001 * elem, in_ld=2000, out_ld=2000)
                batch(R, t, variant, f, 1, 1000, 0, d_out=IN + 500 * elem)
                batch(R, t, variant, f, 4, 10, 0, in_ld=5)                                 # two faults: the first in order wins
                batch(R, t, variant, f, 4, (1 << 30) + 1000, 0, in_ld=100, d_out=IN)
                batch(R, t, variant, f, 0, (1 << 30) + 1000, 0, d_out=IN)
                batch(R, t, variant, None, 4, 10, 0x1000)
                batch(R, t, variant, f, 4, 1000, 0x1000)
                batch(R, t, variant, f, 4, 1000, NARROW | WIDE)
                batch(R, t, variant, f, 4, 1000, AWARE)                                     # known, without effect here
            add(f"E/refusals/{t}/{variant}", fn)
    def fn(R):
        for n, m, d in ((5, 2, 0), (5, 3, 1), (28, 4, 0)):
            f = SavgolFilter()
            C.memmove(C.byref(f), R.filt(n, m, d), C.sizeof(SavgolFilter))
            f.center_weights[1] = 0.25                                                      # a hand-edited table that is not (anti)symmetric
            for t in ("f32", "f64"):
                for variant in ("full", "valid"):
                    for flags in (0, M64, PLAIN):
                        batch(R, t, variant, C.byref(f), 4, 1000, flags)
        g = SavgolFilter()
        C.memmove(C.byref(g), R.filt(5, 2, 0), C.sizeof(SavgolFilter))
        g.window_size = 13
        for t in ("f32", "f64"):
            batch(R, t, "full", C.byref(g), 4, 1000, 0)
        g.window_size = 11
        g.config.half_window = 0
        batch(R, "f32", "full", C.byref(g), 4, 1000, 0)
        g.config.half_window = 33
        batch(R, "f32", "valid", C.byref(g), 4, 1000, 0)
    add("E/hand-edited-tables", fn)

    # ---- F. fp64 with the tolerance in the call -------------------------------------------------------------------------------------------------
    for n in (20, 23, 24, 28, 32):
        for m, d, dt in configs(n, ((2, 0), (3, 1), (4, 2))):
            for variant in ("full", "valid"):
                def fn(R, n=n, m=m, d=d, dt=dt, variant=variant):
                    name = f"savgol_apply{'_valid' if variant == 'valid' else ''}_batch_f64_tol"
                    for mode in (0, 1):
                        for ch, L in ((4, 1000), (4096, 1 << 20)):
                            for tol in (1e-6, 1e-9, 1e-3, 0.0, float("nan"), -1.0):
                                R.call(name, R.filt(n, m, d, dt, mode), IN, OUT, ch, L, L, L, tol, STREAM, note=f"ch={ch} L={L} tol={tol!r}")
                    R.call(name, R.filt(n, m, d, dt, 0), IN, IN, 4, 8192, 8192, 8192, 1e-6, STREAM, note="in place")
                    R.call(name, None, IN, OUT, 4, 1000, 1000, 1000, 1e-6, STREAM, note="NULL filter")
                add(f"F/f64_tol/n{n}/m{m}d{d}dt{dt}/{variant}", fn)
    def fn(R):
        # the tolerance call takes the process defaults for everything but the moment flag
        f = R.filt(28, 2, 0)
        for option, value in ((OPT_TILE, 1), (OPT_TILE, 2), (OPT_CLE, 1), (OPT_PLAIN, 1), (OPT_REF, 1)):
            R.option(option, value)
            try:
                for tol in (1e-6, 1e-9):
                    R.call("savgol_apply_batch_f64_tol", f, IN, OUT, 4, 1000, 1000, 1000, tol, STREAM, note=f"option {option}={value} tol={tol!r}")
                    R.call("savgol_apply_batch_f64_tol", R.filt(12, 3, 1), IN, OUT, 4, 1000, 1000, 1000, tol, STREAM, note=f"n12 option {option}={value} tol={tol!r}")
            finally:
                R.option(option, 0)
    add("F/f64_tol/process-defaults", fn)

    # ---- G. 16-bit storage ----------------------------------------------------------------------------------------------------------------------
    def h16(R, variant, f, in_type, out_type, ch=4, L=1000, flags=0, d_in=IN, d_out=OUT, in_ld=None, out_ld=None):
        R.call(f"savgol_apply{'_valid' if variant == 'valid' else ''}_batch_h16", f, d_in, in_type, d_out, out_type, ch, L, L if in_ld is None else in_ld,
               L if out_ld is None else out_ld, flags, STREAM, note=f"{in_type}->{out_type} ch={ch} L={L} in_ld={in_ld} out_ld={out_ld} flags={flags:#x}")
    PAIRS = ((F16, F16), (BF16, BF16), (F16, F32), (BF16, F32))
    for n in HALF_WINDOWS:
        for m, d, dt in configs(n):
            for variant, mode in (("full", 0), ("full", 1), ("full", 3), ("full", 300), ("valid", 0)):
                def fn(R, n=n, m=m, d=d, dt=dt, variant=variant, mode=mode):
                    for it, ot in PAIRS:
                        for flags in (0, PLAIN, NARROW, CLE):
                            h16(R, variant, R.filt(n, m, d, dt, mode), it, ot, flags=flags)
                add(f"G/h16/n{n}/m{m}d{d}dt{dt}/{variant}/mode{mode}", fn)
    def fn(R):
        for n, m, d, dt in ((4, 2, 0, 1.0), (32, 3, 1, 0.5)):
            f = R.filt(n, m, d, dt)
            for it, ot in PAIRS:
                ob = 4 if ot == F32 else 2
                for variant in ("full", "valid"):
                    h16(R, variant, f, it, ot, 3, 70000, in_ld=70001, out_ld=70003)
                    h16(R, variant, f, it, ot, 3, 70000, in_ld=70004, out_ld=70008, d_in=IN + 2, d_out=OUT + ob)
                    h16(R, variant, f, it, ot, 3, 70000, in_ld=70004, out_ld=70008, d_in=IN + 8, d_out=OUT + 8)       # 8-byte aligned: enough for 16-bit rows only
                    h16(R, variant, f, it, ot, 30000000, 100)
                    h16(R, variant, f, it, ot, 4096, 1 << 20)
                    h16(R, variant, f, it, ot, 4, 1000, d_in=IN, in_ld=2000, d_out=IN + 2 * 1000, out_ld=2000 * 2 // ob)   # interleaved rows (equal byte pitch)
    add("G/h16/shapes", fn)
    for variant in ("full", "valid"):
        def fn(R, variant=variant):
            f = R.filt(5, 2, 0)
            for kw in (dict(flags=REF), dict(flags=WIDE), dict(flags=WIDE | NARROW), dict(flags=AWARE), dict(flags=M64), dict(flags=0x1000),
                       dict(in_type=F32, out_type=F32), dict(in_type=F32, out_type=F16), dict(in_type=F32, out_type=BF16), dict(in_type=F16, out_type=BF16),
                       dict(in_type=BF16, out_type=F16), dict(in_type=3, out_type=F32), dict(in_type=F16, out_type=7), dict(f=None), dict(d_in=None),
                       dict(d_out=None), dict(L=10), dict(in_ld=999), dict(out_ld=500), dict(out_ld=989), dict(out_ld=990), dict(L=(1 << 30) + 1, ch=1),
                       dict(L=(1 << 30) + 1, ch=1, in_ld=100), dict(L=(1 << 30) + 1, f=None), dict(L=10, in_ld=5), dict(L=(1 << 30) + 1, ch=0),      # two faults: the first in order wins
                       dict(ch=0), dict(d_out=IN), dict(d_out=IN + 2), dict(d_out=IN + 4 * 1000 * 2 - 2), dict(d_out=IN - 3 * 1000 * 4 - 4, out_type=F32),
                       dict(d_in=IN, in_ld=2000, d_out=IN + 2 * 999, out_ld=2000)):
                kw = dict(kw)
                it = kw.pop("in_type", F16)
                h16(R, variant, kw.pop("f", f), it, kw.pop("out_type", it), **kw)
            g = SavgolFilter()
            C.memmove(C.byref(g), f, C.sizeof(SavgolFilter))
            g.window_size = 13
            h16(R, variant, C.byref(g), F16, F16)
        add(f"G/h16/refusals/{variant}", fn)

    # ---- H. several filters on one read --------------------------------------------------------------------------------------------------------
    def multi(R, variant, filters, outs, ch=4, L=1000, flags=0, d_in=IN, in_ld=None, out_ld=None, count=None, note=""):
        FP = C.POINTER(SavgolFilter)
        fs = None if filters is None else (FP * max(len(filters), 1))(*[f if f is not None else FP() for f in filters])
        os_ = None if outs is None else (C.c_void_p * max(len(outs), 1))(*outs)
        count = len(filters) if count is None else count
        R.call(f"savgol_apply{'_valid' if variant == 'valid' else ''}_multi_batch_f32", fs, count, d_in, os_, ch, L, L if in_ld is None else in_ld,
               L if out_ld is None else out_ld, flags, STREAM, note=f"count={count} ch={ch} L={L} in_ld={in_ld} out_ld={out_ld} flags={flags:#x} {note}")
    OUTS = (OUT, OUT1, OUT2, OUT3)
    # (poly_order, derivative, time_step) of outputs 0..3: smoothing and derivatives mixed, a derivative first, two smoothing filters
    MIXES = (((2, 0, 1.0), (3, 1, 0.5), (4, 2, 0.5), (4, 0, 1.0)), ((3, 1, 1.0), (2, 0, 1.0), (4, 0, 1.0), (4, 2, 1.0)), ((2, 1, 0.5), (2, 2, 0.5), (2, 1, 1.0), (2, 0, 1.0)))
    for n in (4, 12, 13, 18, 19, 23, 32):
        for mi, mix in enumerate(MIXES):
            for variant, mode in (("full", 0), ("full", 1), ("full", 300), ("valid", 0)):
                for sname, kw in (("4x1000", dict(ch=4, L=1000)), ("4096x2^20", dict(ch=4096, L=1 << 20)), ("16384x1000", dict(ch=16384, L=1000)),
                                  ("16383x1000", dict(ch=16383, L=1000))):
                    def fn(R, n=n, mix=mix, variant=variant, mode=mode, kw=kw):
                        fs = [R.filt(n, m, d, dt, mode) for m, d, dt in mix]
                        for count in (1, 2, 3, 4):
                            for flags in (0, REF, NARROW, WIDE, CLE, PLAIN):
                                multi(R, variant, fs[:count], OUTS[:count], flags=flags, **kw)
                    add(f"H/multi/n{n}/mix{mi}/{variant}/mode{mode}/{sname}", fn)
    def fn(R):
        for n in (4, 32):
            fs = [R.filt(n, m, d, dt) for m, d, dt in MIXES[0]]
            for variant in ("full", "valid"):
                for count in (2, 3, 4):
                    multi(R, variant, fs[:count], OUTS[:count], 30000000, 100)                    # split over channels, the edge items of every output counted
                    multi(R, variant, fs[:count], OUTS[:count], 2, (1 << 30) + 1000)              # single calls, each on its long-channel route
                    multi(R, variant, fs[:count], [OUT + 4, OUT1 + 8, OUT2 + 16, OUT3 + 4][:count], 3, 70000, d_in=IN + 4, in_ld=70004, out_ld=70008)
                    multi(R, variant, fs[:count], OUTS[:count], 3, 70000, in_ld=70001, out_ld=70003)
    add("H/multi/shapes", fn)
    for variant in ("full", "valid"):
        def fn(R, variant=variant):
            a, b, c = R.filt(5, 2, 0), R.filt(5, 3, 1), R.filt(5, 4, 2)
            multi(R, variant, None, [OUT], count=1)
            multi(R, variant, [a, None], [OUT, OUT1])
            multi(R, variant, [a, b], [OUT, OUT1], d_in=None)
            multi(R, variant, [a, b], None)
            multi(R, variant, [a, b], [OUT, None])
            multi(R, variant, [a, b], [OUT, OUT1], count=0)
            multi(R, variant, [a, b, c, a, b], [OUT, OUT1, OUT2, OUT3, OUT3 + (1 << 36)])
            multi(R, variant, [a, R.filt(6, 3, 1)], [OUT, OUT1])
            multi(R, variant, [a, R.filt(5, 3, 1, 1.0, 1)], [OUT, OUT1])
            multi(R, variant, [a, b], [OUT, OUT1], L=10)
            multi(R, variant, [a, b], [OUT, OUT1], in_ld=999)
            multi(R, variant, [a, b], [OUT, OUT1], out_ld=989)
            multi(R, variant, [a, b], [OUT, OUT1], out_ld=990)
            multi(R, variant, [a, b], [OUT, OUT1], ch=0)
            multi(R, variant, [a, b], [OUT, OUT + 400])
            multi(R, variant, [a, b, c], [OUT, OUT1, OUT])
            multi(R, variant, [a, b], [OUT, IN])
            multi(R, variant, [a, b], [IN + 4, OUT1])
            multi(R, variant, [a, b], [OUT, OUT + 4 * 1000], in_ld=2000, out_ld=2000)            # interleaved outputs: no overlap
            multi(R, variant, [a, b], [IN + 4 * 1000, OUT], in_ld=2000, out_ld=2000)             # an output interleaved with the input: none either
            multi(R, variant, [a, b], [OUT, OUT1], flags=NARROW | WIDE)
            multi(R, variant, [a, b], [OUT, OUT1], flags=0x1000)
            g = SavgolFilter()
            C.memmove(C.byref(g), b, C.sizeof(SavgolFilter))
            g.window_size = 13
            multi(R, variant, [a, C.pointer(g)], [OUT, OUT1])
        add(f"H/multi/refusals/{variant}", fn)

    # ---- I. array-of-structs batches ----------------------------------------------------------------------------------------------------------------
    def strided(R, f, flags, in_stride=16, in_off=4, in_pitch=None, out_stride=16, out_off=12, out_pitch=None, ch=3, count=4000, d_in=IN, d_out=IN, ex=True, note=""):
        in_pitch = count * in_stride if in_pitch is None else in_pitch
        out_pitch = count * out_stride if out_pitch is None else out_pitch
        args = [f, d_in, in_stride, in_off, in_pitch, d_out, out_stride, out_off, out_pitch, ch, count]
        R.call("savgol_apply_strided_batch_f32" + ("_ex" if ex else ""), *args, *([flags] if ex else []), STREAM,
               note=f"stride={in_stride},{out_stride} off={in_off},{out_off} pitch={in_pitch},{out_pitch} ch={ch} count={count} flags={flags:#x} {note}")
    for n in (1, 4, 14, 15, 23, 32):
        for m, d, dt in configs(n, ((2, 0), (3, 1))):
            for mode in (0, 1, 3, 300):
                def fn(R, n=n, m=m, d=d, dt=dt, mode=mode):
                    f = R.filt(n, m, d, dt, mode)
                    for flags in (0, AWARE, CLE, AWARE | CLE, REF, REF | AWARE, PLAIN, WIDE):
                        strided(R, f, flags)                                           # two fields of one record array: the fused kernel
                        strided(R, f, flags, out_off=4)                                # the same field in place: staged
                        strided(R, f, flags, d_out=OUT)                                # two arrays
                        strided(R, f, flags, in_stride=10, in_off=2, d_out=OUT)        # unaligned: staged
                        strided(R, f, flags, out_off=6)                                # fields that share bytes: staged
                add(f"I/strided/n{n}/m{m}d{d}dt{dt}/mode{mode}", fn)
    def fn(R):
        f = R.filt(4, 2, 0)
        for flags in (0, AWARE):
            strided(R, f, flags, in_stride=8, in_off=0, out_stride=8, out_off=4, ch=30000000, count=100)       # split over channels
            strided(R, f, flags, in_stride=8, in_off=0, out_stride=8, out_off=4, ch=1, count=(1 << 30) + 1000)  # beyond one launch: staged
            strided(R, f, flags, in_stride=8, in_off=0, in_pitch=40000, out_stride=12, out_off=8, out_pitch=60000, d_out=OUT)
            strided(R, f, flags, in_stride=4, in_off=0, out_stride=4, out_off=0, d_out=OUT)
            strided(R, f, flags, in_stride=2, in_off=0, d_out=OUT)
        strided(R, None, 0)
        strided(R, f, 0, d_in=None)
        strided(R, f, 0, d_out=None)
        strided(R, f, 0, count=8)
        strided(R, f, 0, ch=0)
        strided(R, f, 0x1000)
        strided(R, f, NARROW | WIDE)
        g = SavgolFilter()
        C.memmove(C.byref(g), f, C.sizeof(SavgolFilter))
        g.window_size = 13
        strided(R, C.byref(g), 0)
    add("I/strided/shapes-and-refusals", fn)

    # ---- J. the default-flag entry points under every process option ----------------------------------------------------------------------------
    for option, value in ((None, 0), (OPT_CLE, 1), (OPT_REF, 1), (OPT_PLAIN, 1), (OPT_AWARE, 1), (OPT_TILE, 1), (OPT_TILE, 2)):
        for n, m, d, dt, mode in ((4, 2, 0, 1.0, 0), (12, 3, 1, 0.5, 0), (18, 3, 1, 0.5, 1), (23, 2, 0, 1.0, 0), (32, 3, 1, 0.5, 0), (32, 4, 0, 1.0, 2)):
            def fn(R, option=option, value=value, n=n, m=m, d=d, dt=dt, mode=mode):
                f = R.filt(n, m, d, dt, mode)
                if option is not None:
                    R.option(option, value)
                try:
                    for ch, L in ((4, 1000), (4096, 1 << 20)):
                        for t in ("f32", "f64"):
                            for variant in ("full", "valid"):
                                R.call(batch_name(t, variant, ex=False), f, IN, OUT, ch, L, L, L, STREAM, note=f"ch={ch} L={L}")
                    R.call("savgol_apply_batch_f32", f, IN, IN, 4, 8192, 8192, 8192, STREAM, note="in place")
                    R.call("savgol_apply_batch_f32", None, IN, OUT, 4, 1000, 1000, 1000, STREAM, note="NULL filter")
                    strided(R, f, 0, ex=False)
                    strided(R, f, 0, ex=False, out_off=4)
                    R.rcs.append(int(R.lib.savgol_hip_default_flags()))
                finally:
                    if option is not None:
                        R.option(option, 0)
            add(f"J/defaults/option{option}={value}/n{n}m{m}d{d}/mode{mode}", fn)

    # ---- K. the host-pointer drop-ins: small service -> zero copy -> arena ---------------------------------------------------------------------------
    for length in (360, 3000, 4096, 4097, 2047, 2048, 100000, 262144, 262145, 500000):
        for n, m, d, dt, mode in ((4, 2, 0, 1.0, 0), (12, 3, 1, 0.5, 0), (12, 3, 1, 0.5, 1), (32, 4, 0, 1.0, 3)):
            def fn(R, length=length, n=n, m=m, d=d, dt=dt, mode=mode):
                f = R.filt(n, m, d, dt, mode)
                x = np.zeros(length, np.float32)
                y = np.zeros(length, np.float32)
                aos_in = np.zeros((length, 3), np.float32)
                aos_out = np.zeros((length, 2), np.float32)
                R.bases([("hin", x.ctypes.data, x.nbytes), ("hout", y.ctypes.data, y.nbytes), ("aos_in", aos_in.ctypes.data, aos_in.nbytes),
                         ("aos_out", aos_out.ctypes.data, aos_out.nbytes)])
                for option in (None, OPT_CLE, OPT_AWARE, OPT_REF, OPT_PLAIN):
                    if option is not None:
                        R.option(option, 1)
                    try:
                        for small in (1, 0):
                            R.lib.rec_set_small(small)
                            note = f"L={length} option={option} small={small}"
                            R.call("savgol_apply", f, x.ctypes.data, y.ctypes.data, length, note=note)
                            R.call("savgol_apply", f, x.ctypes.data, x.ctypes.data, length, note=note + " in place")
                            R.call("savgol_apply_valid", f, x.ctypes.data, length, y.ctypes.data, note=note)
                            R.call("savgol_apply_strided", f, aos_in.ctypes.data, 12, 4, aos_out.ctypes.data, 8, 4, length, note=note)
                    finally:
                        R.lib.rec_set_small(0)
                        if option is not None:
                            R.option(option, 0)
            add(f"K/host/L{length}/n{n}m{m}d{d}/mode{mode}", fn)
    def fn(R):
        f = R.filt(5, 2, 0)
        x = np.zeros(1000, np.float32)
        y = np.zeros(1000, np.float32)
        R.bases([("hin", x.ctypes.data, x.nbytes), ("hout", y.ctypes.data, y.nbytes)])
        xp, yp = x.ctypes.data, y.ctypes.data
        for args in ((None, xp, yp, 1000), (f, None, yp, 1000), (f, xp, None, 1000), (f, xp, yp, 10), (f, xp, yp, 11)):
            R.call("savgol_apply", *args)
        for args in ((None, xp, 1000, yp), (f, None, 1000, yp), (f, xp, 1000, None), (f, xp, 10, yp), (f, xp, 11, yp)):
            R.call("savgol_apply_valid", *args)
        for args in ((None, xp, 8, 0, yp, 8, 4, 100), (f, None, 8, 0, yp, 8, 4, 100), (f, xp, 8, 0, None, 8, 4, 100), (f, xp, 8, 0, yp, 8, 4, 10), (f, xp, 8, 0, yp, 8, 4, 11)):
            R.call("savgol_apply_strided", *args)
    add("K/host/refusals", fn)
    return out


SHORT = {"scratch_alloc": "alloc", "scratch_free": "free", "hipStreamSynchronize": "sync", "reference_order_f32": "ref", "refpk_f32": "refpk",
         "hipMemcpy2DAsync": "copy2d", "hipMemcpyAsync": "copy_async", "hipMemcpy": "copy", "ctx_pinned": "pinned", "ctx_arena": "arena", "small_call": "small"}


def run_lengths(items):
    """[(item, count)] of consecutive equal items, then of consecutive equal BLOCKS of up to 96 runs: 'a, b, a, b' -> '(a, b) x2'"""
    runs = []
    for item in items:
        if runs and runs[-1][0] == item:
            runs[-1][1] += 1
        else:
            runs.append([item, 1])
    tokens = [item if k == 1 else f"{item} x{k}" for item, k in runs]
    while True:                                     # passes until nothing folds: blocks of blocks
        out, i = [], 0
        while i < len(tokens):
            for b in range(2, 97):
                k = 1
                while tokens[i + k * b:i + (k + 1) * b] == tokens[i:i + b]:
                    k += 1
                if k > 1:
                    out.append(f"({', '.join(tokens[i:i + b])}) x{k}")
                    i += k * b
                    break
            else:
                out.append(tokens[i])
                i += 1
        if len(out) == len(tokens):
            break
        tokens = out
    return ", ".join(out) or "-"


def short_form(record):
    """the launcher sequence in short form: 'f32_g1 x3, ends x2, ...' (the notes of the calls themselves left out)"""
    names = [line.split(" ", 1)[0] for line in record.splitlines() if line and not line.startswith(("call ", "-> ", "part "))]
    return run_lengths([SHORT.get(name, name) for name in names])


def run_cases(lib):
    """{case id: (golden line, full record)} in generation order"""
    R = Recorder(lib)
    groups = {}
    for pid, fn in cases():
        groups.setdefault("/".join(pid.split("/")[:3]), []).append((pid, fn))
    results = {}
    for cid, parts in groups.items():
        assert "\t" not in cid and len({pid for pid, _ in parts}) == len(parts), cid
        R.begin()
        for pid, fn in parts:
            R.bases()
            lib.rec_note(f"part {pid}".encode())
            fn(R)
        record, rcs = R.end()
        assert "UNKNOWN" not in record, (cid, record)
        sha = hashlib.sha256(record.encode()).hexdigest()
        results[cid] = (f"{cid}\t{len(parts)} parts\t{run_lengths(map(str, rcs))}\t{short_form(record)}\t{sha}", record)
    assert lib.savgol_hip_default_flags() == 0
    return results


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if not os.path.exists(HIP_HEADER):
        pytest.skip("hip/hip_runtime_api.h is not installed")
    # stderr of the drop-in calls' refusals ("savgol_apply: NULL pointer") is theirs by contract; keep it out of the test log
    return run_cases(load(build(str(tmp_path_factory.mktemp("launch_recorder")))))


def golden_lines():
    with open(GOLDEN) as fh:
        return {line.split("\t", 1)[0]: line.rstrip("\n") for line in fh if line.strip()}


def test_case_ids_are_the_golden_ones(results):
    want = golden_lines()
    assert set(results) == set(want), (sorted(set(results) - set(want))[:10], sorted(set(want) - set(results))[:10])
    assert len(want) > 100


def test_launch_record_matches_golden(results):
    want = golden_lines()
    bad = [cid for cid in results if results[cid][0] != want.get(cid)]
    for cid in bad[:3]:
        print(f"==== {cid}\n golden: {want.get(cid)}\n now:    {results[cid][0]}\n---- the full record now:\n{results[cid][1]}")
    assert not bad, f"{len(bad)} of {len(results)} cases differ from tests/golden/launch_record_1d.txt, the first: {bad[:10]}"


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        res = run_cases(load(build(tmp)))
    if "--dump" in sys.argv:
        d = sys.argv[sys.argv.index("--dump") + 1]
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "index.txt"), "w") as index:
            for k, (cid, (line, record)) in enumerate(res.items()):
                index.write(f"{k}\t{line}\n")
                with open(os.path.join(d, f"{k}.txt"), "w") as fh:
                    fh.write(record)
    if "--record" in sys.argv:
        with open(GOLDEN, "w") as fh:
            fh.write("".join(line + "\n" for line, _ in res.values()))
        print(f"wrote {len(res)} cases to {GOLDEN}")
