"""CPU-side checks of the 16-bit-storage 1-D batch call (savgol_apply[_valid]_batch_h16): both symbols are bound with their arity and the storage
constants exported, every refusal returns -1 with its text before any device call (fake device addresses), the call fails loudly without a device,
apply_tensor still refuses dtypes it does not serve, and the library's 71 new kernels carry no private segment.  No GPU needed."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("savgol_apply_batch_h16", "savgol_apply_valid_batch_h16")

# fake device addresses: the checks run before anything touches them
IN, OUT = 0x100000000, 0x200000000


def call(sg, name, f, d_in=IN, in_type=None, d_out=OUT, out_type=None, channels=4, length=1000, in_ld=None, out_ld=None, flags=0):
    in_type = sg.SAVGOL_HIP_F16 if in_type is None else in_type
    out_type = in_type if out_type is None else out_type
    return getattr(sg.lib(), name)(None if f is None else f.ptr, d_in, in_type, d_out, out_type, channels, length,
                                   length if in_ld is None else in_ld, length if out_ld is None else out_ld, flags, None)


def test_h16_symbols_bound(sg):
    for name in NAMES:
        assert name in sg.SIGNATURES
        assert len(getattr(sg.lib(), name).argtypes) == 11
    assert (sg.SAVGOL_HIP_F32, sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16) == (0, 1, 2)


@pytest.mark.parametrize("name", NAMES)
def test_h16_refusals_need_no_device(sg, name):
    f = sg.Filter(5, 2, 0)
    F32, F16, BF16 = sg.SAVGOL_HIP_F32, sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_BF16
    cases = [
        ({"flags": sg.SAVGOL_BATCH_REFERENCE_SUMMATION}, "SAVGOL_BATCH_REFERENCE_SUMMATION is not served"),
        ({"flags": sg.SAVGOL_BATCH_TILE_WIDE}, "SAVGOL_BATCH_TILE_WIDE is not served"),
        ({"flags": sg.SAVGOL_BATCH_TILE_WIDE | sg.SAVGOL_BATCH_TILE_NARROW}, "SAVGOL_BATCH_TILE_WIDE is not served"),
        ({"flags": sg.SAVGOL_BATCH_BOUNDARY_AWARE}, "belong to other calls"),
        ({"flags": sg.SAVGOL_BATCH_MOMENT_F64}, "belong to other calls"),
        ({"flags": 0x1000}, "bad flags 0x1000"),
        ({"in_type": F32, "out_type": F32}, "f32 -> f32"),
        ({"in_type": F32, "out_type": F16}, "f32 -> f16"),
        ({"in_type": F32, "out_type": BF16}, "f32 -> bf16"),
        ({"in_type": F16, "out_type": BF16}, "f16 -> bf16"),
        ({"in_type": BF16, "out_type": F16}, "bf16 -> f16"),
        ({"in_type": 3, "out_type": F32}, "unknown -> f32"),
        ({"in_type": F16, "out_type": 7}, "f16 -> unknown"),
        ({"f": None}, "NULL pointer"),
        ({"d_in": None}, "NULL pointer"),
        ({"d_out": None}, "NULL pointer"),
        ({"length": 10}, "data length (10) < window size (11)"),
        ({"in_ld": 999}, "row pitch smaller than the row"),
        ({"out_ld": 500}, "row pitch smaller than the row"),
        ({"length": (1 << 30) + 1, "channels": 1}, "channels longer than 2^30 samples"),
        ({"d_out": IN}, "d_in and d_out overlap"),                                         # in place
        ({"d_out": IN + 2}, "d_in and d_out overlap"),                                      # shifted by one element
        ({"d_out": IN + 4 * 1000 * 2 - 2}, "d_in and d_out overlap"),                       # the input's last element
        ({"d_out": IN - 3 * 1000 * 4 - 4, "out_type": F32}, "d_in and d_out overlap"),      # an fp32 output whose last row starts one element before the input
        ({"d_in": IN, "in_ld": 2000, "d_out": IN + 2 * 999, "out_ld": 2000}, "d_in and d_out overlap"),   # interleaved rows, one byte pair shared
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc = call(sg, name, kw.pop("f", f), **kw)
        assert rc == -1, (text, rc)
        assert text in sg.last_error(), (text, sg.last_error())
        assert name in sg.last_error()
    if name == NAMES[1]:
        # VALID: the output row is length - 2n long
        assert call(sg, name, f, out_ld=989) == -1 and "row pitch smaller than the row" in sg.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_h16_interleaved_rows_are_not_an_overlap(sg, name):
    """in = buf[:, 0, :], out = buf[:, 1, :] with both pitches 2 L touch no common byte: the argument checks pass (zero channels: nothing to enqueue)"""
    f = sg.Filter(5, 2, 0)
    assert call(sg, name, f, channels=0) == 0
    if sg.device_count() == 0:
        assert call(sg, name, f, d_in=IN, in_ld=2000, d_out=IN + 2 * 1000, out_ld=2000) == -1
        assert "no usable HIP device" in sg.last_error()


def test_h16_no_cpu_fallback_without_device(sg):
    """With valid arguments and no GPU the call must FAIL, not compute on the host"""
    if sg.device_count() > 0:
        pytest.skip("a GPU is present")
    f = sg.Filter(5, 4, 1)
    for name in NAMES:
        for it, ot in ((sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_F16), (sg.SAVGOL_HIP_BF16, sg.SAVGOL_HIP_BF16), (sg.SAVGOL_HIP_F16, sg.SAVGOL_HIP_F32),
                       (sg.SAVGOL_HIP_BF16, sg.SAVGOL_HIP_F32)):
            assert call(sg, name, f, in_type=it, out_type=ot) == -1
            assert "no usable HIP device" in sg.last_error()
    with pytest.raises(RuntimeError):
        f.apply_batch(IN, OUT, 4, 1000, dtype="bf16", out_dtype="f32")


def test_apply_tensor_refuses_unserved_dtypes(sg):
    import torch
    f = sg.Filter(5, 2, 0)
    for dt in (torch.int16, torch.int32, torch.uint8):
        with pytest.raises(TypeError):
            f.apply_tensor(torch.zeros((2, 100), dtype=dt))
    for dt, out in ((torch.float32, torch.float16), (torch.float16, torch.bfloat16), (torch.float64, torch.float32), (torch.bfloat16, torch.float16)):
        with pytest.raises(TypeError):
            f.apply_tensor(torch.zeros((2, 100), dtype=dt), out_dtype=out)


def test_h16_kernels_in_the_library_have_no_private_segment():
    lib = os.path.join(ROOT, "savitzky-golay-filter_amd", "lib", "libsavgol_hip.so")
    if not (os.path.exists(lib) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("library or llvm-readelf not present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), lib, "sg1d_h16_"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    plain, moment = {}, {}
    for line in out.stdout.splitlines():
        m = re.match(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) spill\s+(\d+) lds\s+(\d+)\s+.*sg1d_h16_(momenth_)?kernel<(\d+)(?:, (\d+))?>", line)
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
