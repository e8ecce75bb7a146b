"""CPU-side checks of the fused multi-output 1-D call (savgol_apply[_valid]_multi_batch_f32): every argument error returns -1 with its text
before any device call, the call fails loudly without a device, the Python mirror binds both symbols, and the library carries the 64 fused
kernels without a private segment.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("savgol_apply_multi_batch_f32", "savgol_apply_valid_multi_batch_f32")

# fake device addresses: the checks run before anything touches them
IN, OUT0, OUT1, OUT2 = 0x100000000, 0x200000000, 0x300000000, 0x400000000


def call(sg, name, filters, d_in, d_outs, channels=4, length=1000, in_ld=None, out_ld=None, flags=0, count=None):
    F = C.POINTER(sg.SavgolFilter)
    fs = None if filters is None else (F * max(len(filters), 1))(*[f.ptr if f is not None else F() for f in filters])
    outs = None if d_outs is None else (C.c_void_p * max(len(d_outs), 1))(*d_outs)
    count = len(filters) if count is None else count
    return getattr(sg.lib(), name)(fs, count, d_in, outs, channels, length, length if in_ld is None else in_ld,
                                   length if out_ld is None else out_ld, flags, None)


def test_multi_symbols_bound(sg):
    for name in NAMES:
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == 10
    assert callable(sg.apply_multi_batch) and callable(sg.apply_multi_tensor)
    assert sg.SAVGOL_MULTI_MAX_FILTERS == 4


@pytest.mark.parametrize("name", NAMES)
def test_multi_argument_errors_need_no_device(sg, name):
    a, b, c = sg.Filter(5, 2, 0), sg.Filter(5, 3, 1), sg.Filter(5, 4, 2)
    cases = [
        ((None, IN, [OUT0]), {"count": 1}, "NULL pointer"),
        (([a, None], IN, [OUT0, OUT1]), {}, "NULL pointer"),
        (([a, b], None, [OUT0, OUT1]), {}, "NULL pointer"),
        (([a, b], IN, None), {}, "NULL pointer"),
        (([a, b], IN, [OUT0, None]), {}, "NULL pointer"),
        (([a, b], IN, [OUT0, OUT1]), {"count": 0}, "count 0 outside 1..4"),
        (([a, b, c, a, b], IN, [OUT0, OUT1, OUT2, OUT0 + 0x10000000, OUT1 + 0x10000000]), {}, "count 5 outside 1..4"),
        (([a, sg.Filter(6, 3, 1)], IN, [OUT0, OUT1]), {}, "half_window"),
        (([a, sg.Filter(5, 3, 1, 1.0, sg.SAVGOL_BOUNDARY_REFLECT)], IN, [OUT0, OUT1]), {}, "boundary"),
        (([a, b], IN, [OUT0, OUT1]), {"length": 10}, "data length (10) < window size (11)"),
        (([a, b], IN, [OUT0, OUT1]), {"in_ld": 999}, "row pitch smaller than the row"),
        (([a, b], IN, [OUT0, OUT0 + 400]), {}, "d_outs[0] and d_outs[1] overlap"),
        (([a, b, c], IN, [OUT0, OUT1, OUT0]), {}, "d_outs[0] and d_outs[2] overlap"),
        (([a, b], IN, [OUT0, IN]), {}, "d_outs[1] overlaps d_in (the multi-output call does not run in place)"),
        (([a, b], IN, [IN + 4, OUT1]), {}, "d_outs[0] overlaps d_in"),
    ]
    for (filters, d_in, d_outs), kw, text in cases:
        rc = call(sg, name, filters, d_in, d_outs, **kw)
        assert rc == -1, (text, rc)
        assert text in sg.last_error(), (text, sg.last_error())
        assert name in sg.last_error()


def test_multi_bad_flags(sg):
    a, b = sg.Filter(5, 2, 0), sg.Filter(5, 3, 1)
    assert call(sg, NAMES[0], [a, b], IN, [OUT0, OUT1], flags=sg.SAVGOL_BATCH_TILE_NARROW | sg.SAVGOL_BATCH_TILE_WIDE) == -1
    assert "bad flags" in sg.last_error()


def test_multi_no_cpu_fallback_without_device(sg):
    """With valid arguments and no GPU the call must FAIL, not compute on the host (as test_no_cpu_fallback_without_device)."""
    if sg.device_count() > 0:
        pytest.skip("a GPU is present")
    fs = [sg.Filter(5, 4, d) for d in range(3)]
    for name in NAMES:
        for count in (1, 2, 3):
            assert call(sg, name, fs[:count], IN, [OUT0, OUT1, OUT2][:count]) == -1
            assert "no usable HIP device" in sg.last_error()
        with pytest.raises(RuntimeError):
            sg.apply_multi_batch(fs, IN, [OUT0, OUT1, OUT2], 4, 1000, valid=name == NAMES[1])


def test_multi_kernels_in_the_library_have_no_private_segment():
    lib = os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")
    if not (os.path.exists(lib) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("library or llvm-readelf not present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), lib, "sg1d_multi_kernel"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) spill\s+(\d+) lds\s+(\d+)\s+.*sg1d_multi_kernel<(\d+), (\d+)>", line)
        if m:
            rows[(int(m.group(6)), int(m.group(7)))] = (int(m.group(3)), int(m.group(4)), int(m.group(1)))
    assert set(rows) == {(n, k) for n in range(1, 33) for k in (2, 3)}, sorted(rows)
    for key, (scratch, spill, vgpr) in rows.items():
        assert scratch == 0 and spill == 0, (key, scratch, spill)
        assert vgpr <= 256, (key, vgpr)                      # 2 waves per SIMD
    assert rows[(32, 3)][:2] == (0, 0)
