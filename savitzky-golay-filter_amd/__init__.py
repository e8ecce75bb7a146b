"""savgol_amd -- Python mirror (ctypes) of the C ABI of libsavgol_hip.so.

The product is the shared library: host C/C++ that keeps the reference's savgolFilter.h /
savgol_stream.h / savgol2d.h API, and hand-written gfx950 HIP kernels for the hot path.  This module
only binds it: same function names, same argument meaning and error behaviour as the C headers in
../include (which cite the reference lines they replace).  There is no Python or CPU compute path
in here -- if the library is missing, importing `lib()` fails loudly.

Host-pointer calls take numpy arrays; device-pointer calls take anything with `.data_ptr()`
(torch tensors: torch is used for device memory / streams only) or a raw integer address.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAVGOL_HIP_LIB: another build of the same library (tools/ A/B runs); the product is lib/libsavgol_hip.so
LIB_PATH = os.environ.get("SAVGOL_HIP_LIB") or os.path.join(_HERE, "lib", "libsavgol_hip.so")

SAVGOL_MAX_HALF_WINDOW = 32
SAVGOL_MAX_WINDOW = 65
SAVGOL_MAX_POLY_ORDER = 10
SAVGOL_MAX_DERIVATIVE = 4
SAVGOL_BOUNDARY_POLYNOMIAL, SAVGOL_BOUNDARY_REFLECT, SAVGOL_BOUNDARY_PERIODIC, SAVGOL_BOUNDARY_CONSTANT = 0, 1, 2, 3
SAVGOL2D_BOUNDARY_VALID, SAVGOL2D_BOUNDARY_CONSTANT, SAVGOL2D_BOUNDARY_REFLECT = 0, 1, 2
SAVGOL_HIP_OPT_CORRECT_LEADING_EDGE = 1
SAVGOL_HIP_OPT_REFERENCE_SUMMATION = 2
SAVGOL_HIP_OPT_PLAIN_SUMMATION = 3
SAVGOL_HIP_OPT_BOUNDARY_AWARE = 4
SAVGOL_HIP_OPT_TILE_WIDTH = 5
SAVGOL_STREAMBANK_FMA = 1
SAVGOL_BATCH_REFERENCE_SUMMATION, SAVGOL_BATCH_PLAIN_SUMMATION, SAVGOL_BATCH_TILE_NARROW, SAVGOL_BATCH_TILE_WIDE = 1, 2, 4, 8
SAVGOL_BATCH_CORRECT_LEADING_EDGE, SAVGOL_BATCH_BOUNDARY_AWARE, SAVGOL_BATCH_MOMENT_F64 = 16, 32, 64
SAVGOL_MULTI_MAX_FILTERS = 4
SAVGOL_STRIDED_MULTI_MAX_JOBS = 16
SAVGOL_HIP_F32, SAVGOL_HIP_F16, SAVGOL_HIP_BF16 = 0, 1, 2          # storage type of a device buffer (savgol_apply[_valid]_batch_h16)
_STORAGE = {"f32": SAVGOL_HIP_F32, "f16": SAVGOL_HIP_F16, "bf16": SAVGOL_HIP_BF16}
SAVGOL_HIP_I16 = 3                                                  # int16 samples (savgol_apply[_valid]_batch_i16); not a type of the 16-bit float calls


class SavgolConfig(C.Structure):
    _fields_ = [("half_window", C.c_uint8), ("poly_order", C.c_uint8), ("derivative", C.c_uint8),
                ("time_step", C.c_float), ("boundary", C.c_int)]


class SavgolFilter(C.Structure):
    _fields_ = [("config", SavgolConfig), ("window_size", C.c_int), ("dt_scale", C.c_float),
                ("center_weights", C.c_float * SAVGOL_MAX_WINDOW),
                ("edge_weights", (C.c_float * SAVGOL_MAX_WINDOW) * SAVGOL_MAX_HALF_WINDOW)]


class SavgolFieldJob(C.Structure):
    _fields_ = [("filter", C.POINTER(SavgolFilter)), ("in_offset", C.c_size_t), ("out_offset", C.c_size_t)]


class SavgolStream(C.Structure):
    _fields_ = [("filter", C.POINTER(SavgolFilter)), ("buffer", C.c_float * SAVGOL_MAX_WINDOW),
                ("write_pos", C.c_int), ("samples_received", C.c_size_t), ("samples_output", C.c_size_t),
                ("owns_filter", C.c_bool), ("dt_inv", C.c_float)]


class Savgol2DConfig(C.Structure):
    _fields_ = [("half_window_x", C.c_uint8), ("half_window_y", C.c_uint8), ("poly_order", C.c_uint8),
                ("deriv_x", C.c_uint8), ("deriv_y", C.c_uint8), ("delta_x", C.c_float), ("delta_y", C.c_float)]


class Savgol2DFilter(C.Structure):
    _fields_ = [("config", Savgol2DConfig), ("window_width", C.c_int), ("window_height", C.c_int),
                ("window_area", C.c_int), ("num_terms", C.c_int), ("scale", C.c_float),
                ("weights", C.POINTER(C.c_float))]


_fp, _dp, _vp, _sz = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p, C.c_size_t
_F, _F2, _S = C.POINTER(SavgolFilter), C.POINTER(Savgol2DFilter), C.POINTER(SavgolStream)

# name -> (restype, argtypes); everything include/*.h declares
SIGNATURES = {
    # savgolFilter.h
    "savgol_create": (_F, [C.POINTER(SavgolConfig)]),
    "savgol_destroy": (None, [_F]),
    "savgol_apply": (C.c_int, [_F, _fp, _fp, _sz]),
    "savgol_apply_strided": (C.c_int, [_F, _vp, _sz, _sz, _vp, _sz, _sz, _sz]),
    "savgol_apply_valid": (_sz, [_F, _fp, _sz, _fp]),
    # savgol_stream.h
    "savgol_stream_create": (_S, [C.POINTER(SavgolConfig)]),
    "savgol_stream_init": (C.c_int, [_S, _F]),
    "savgol_stream_destroy": (None, [_S]),
    "savgol_stream_reset": (None, [_S]),
    "savgol_stream_push": (C.c_float, [_S, C.c_float, C.POINTER(C.c_bool)]),
    "savgol_stream_push_full": (C.c_int, [_S, C.c_float, _fp, C.c_int]),
    "savgol_stream_flush": (C.c_int, [_S, _fp, C.c_int]),
    "savgol_stream_flush_leading": (C.c_int, [_S, _fp, C.c_int]),
    "savgol_stream_ready": (C.c_bool, [_S]),
    "savgol_stream_latency": (_sz, [_S]),
    "savgol_stream_buffered": (_sz, [_S]),
    "savgol_stream_samples_received": (_sz, [_S]),
    "savgol_stream_samples_output": (_sz, [_S]),
    # savgol2d.h
    "savgol2d_create": (_F2, [C.POINTER(Savgol2DConfig)]),
    "savgol2d_destroy": (None, [_F2]),
    "savgol2d_config_valid": (C.c_bool, [C.POINTER(Savgol2DConfig)]),
    "savgol2d_apply_valid": (C.c_int, [_F2, _fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int]),
    "savgol2d_apply": (C.c_int, [_F2, _fp, C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_int]),
    "savgol2d_gradient": (C.c_int, [C.c_int] * 3 + [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_float, C.c_float, C.c_int]),
    "savgol2d_hessian": (C.c_int, [C.c_int] * 3 + [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, C.c_float, C.c_float, C.c_int]),
    "savgol2d_laplacian": (C.c_int, [C.c_int] * 3 + [_fp, C.c_int, C.c_int, C.c_int, _fp, C.c_float, C.c_float, C.c_int]),
    # savgol_hip.h: runtime
    "savgol_hip_device_count": (C.c_int, []),
    "savgol_hip_set_device": (C.c_int, [C.c_int]),
    "savgol_hip_get_device": (C.c_int, []),
    "savgol_hip_synchronize": (C.c_int, [_vp]),
    "savgol_hip_trim_scratch": (C.c_int, []),
    "savgol_hip_scratch_reserved": (C.c_size_t, []),
    "savgol_hip_shard_range": (C.c_int, [_sz, C.c_int, C.c_int, C.POINTER(_sz), C.POINTER(_sz)]),
    "savgol_hip_last_error": (C.c_char_p, []),
    "savgol_hip_version": (C.c_char_p, []),
    "savgol_hip_set_option": (C.c_int, [C.c_int, C.c_int]),
    "savgol_hip_momenth_table": (C.c_int, [_F, _fp]),
    "savgol_hip_moment64_table": (C.c_int, [_F, _dp]),
    "savgol_hip_stream_moment_table": (C.c_int, [C.c_int, _fp, _fp]),
    "savgol_export_header": (C.c_long, [_F, C.c_char_p, C.c_char_p, C.c_char_p, _sz]),
    # savgol_hip.h: 1-D batch
    "savgol_apply_batch_f32": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    "savgol_apply_batch_f64": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    "savgol_apply_valid_batch_f32": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    "savgol_apply_valid_batch_f64": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    "savgol_apply_strided_batch_f32": (C.c_int, [_F, _vp, _sz, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _sz, _vp]),
    "savgol_apply_batch_f32_ex": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_batch_f64_ex": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_batch_f64_tol": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, C.c_double, _vp]),
    "savgol_apply_valid_batch_f64_tol": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, C.c_double, _vp]),
    "savgol_apply_valid_batch_f32_ex": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_valid_batch_f64_ex": (C.c_int, [_F, _vp, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_strided_batch_f32_ex": (C.c_int, [_F, _vp, _sz, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_strided_multi_batch_f32": (C.c_int, [C.POINTER(SavgolFieldJob), C.c_int, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_strided_multi_batch_f32_route": (C.c_int, [C.POINTER(SavgolFieldJob), C.c_int, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, C.c_uint]),
    "savgol_apply_multi_batch_f32": (C.c_int, [C.POINTER(_F), C.c_int, _vp, C.POINTER(_vp), _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_valid_multi_batch_f32": (C.c_int, [C.POINTER(_F), C.c_int, _vp, C.POINTER(_vp), _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_batch_h16": (C.c_int, [_F, _vp, C.c_int, _vp, C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_batch_i16": (C.c_int, [_F, _vp, _vp, C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_valid_batch_i16": (C.c_int, [_F, _vp, _vp, C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_multi_batch_h16": (C.c_int, [C.POINTER(_F), C.c_int, _vp, C.c_int, C.POINTER(_vp), C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_valid_multi_batch_h16": (C.c_int, [C.POINTER(_F), C.c_int, _vp, C.c_int, C.POINTER(_vp), C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_multi_batch_i16": (C.c_int, [C.POINTER(_F), C.c_int, _vp, C.POINTER(_vp), C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_valid_multi_batch_i16": (C.c_int, [C.POINTER(_F), C.c_int, _vp, C.POINTER(_vp), C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_apply_valid_batch_h16": (C.c_int, [_F, _vp, C.c_int, _vp, C.c_int, _sz, _sz, _sz, _sz, C.c_uint, _vp]),
    "savgol_hip_default_flags": (C.c_uint, []),
    # savgol_hip.h: stream bank
    "savgol_streambank_create": (_vp, [C.POINTER(SavgolConfig), _sz]),
    "savgol_streambank_create_ex": (_vp, [C.POINTER(SavgolConfig), _sz, C.c_uint]),
    "savgol_streambank_destroy": (None, [_vp]),
    "savgol_streambank_reset": (C.c_int, [_vp, _vp]),
    "savgol_streambank_push": (C.c_int, [_vp, _vp, _vp, _vp]),
    "savgol_streambank_push_wait": (C.c_int, [_vp, _vp, _vp, _vp]),
    "savgol_streambank_push_full": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "savgol_streambank_push_block": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "savgol_streambank_push_block_h16": (C.c_int, [_vp, _vp, C.c_int, _sz, _vp, C.c_int, _vp]),
    "savgol_streambank_push_block_i16": (C.c_int, [_vp, _vp, _sz, _vp, C.c_int, _vp]),
    "savgol_streambank_push_block_multi": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp, C.POINTER(C.c_int), _vp]),
    "savgol_streambank_push_block_multi_route": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp]),
    "savgol_streambank_push_block_multi_h16": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _sz, _vp, C.c_int, C.POINTER(C.c_int), _vp]),
    "savgol_streambank_push_block_multi_h16_route": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _sz, _vp, C.c_int]),
    "savgol_streambank_push_block_multi_i16": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp, C.c_int, C.POINTER(C.c_int), _vp]),
    "savgol_streambank_push_block_multi_i16_route": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp, C.c_int]),
    "savgol_streambank_flush": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "savgol_streambank_flush_leading": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "savgol_streambank_ready": (C.c_bool, [_vp]),
    "savgol_streambank_latency": (_sz, [_vp]),
    "savgol_streambank_streams": (_sz, [_vp]),
    "savgol_streambank_samples_received": (_sz, [_vp]),
    "savgol_streambank_samples_output": (_sz, [_vp]),
    "savgol_streambank_service_start": (C.c_int, [_vp, C.c_uint]),
    "savgol_streambank_service_tick": (C.c_int, [_vp, _vp, _vp]),
    "savgol_streambank_service_stop": (C.c_int, [_vp]),
    "savgol_streambank_service_running": (C.c_int, [_vp]),
    "savgol_streambank_state_bytes": (_sz, [_vp]),
    "savgol_streambank_save": (C.c_int, [_vp, _vp, _vp]),
    "savgol_streambank_load": (C.c_int, [_vp, _vp, _vp]),
    # savgol_hip.h: 2-D batch
    "savgol2d_apply_batch_f32": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, _sz, _vp, C.c_int, _sz, _sz, C.c_int, C.c_int, _vp]),
    "savgol2d_apply_batch_h16": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _sz, _vp, C.c_int, C.c_int, _sz, _sz, C.c_int, C.c_int, _vp]),
    "savgol2d_apply_batch_h16_route": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _sz, _vp, C.c_int, C.c_int, _sz, _sz, C.c_int, C.c_int]),
    "savgol2d_apply_batch_i16": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, _sz, _vp, C.c_int, C.c_int, _sz, _sz, C.c_int, C.c_int, _vp]),
    "savgol2d_apply_batch_i16_route": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, _sz, _vp, C.c_int, C.c_int, _sz, _sz, C.c_int, C.c_int]),
    "savgol2d_gradient_batch_i16": (C.c_int, [C.c_int] * 3 + [_vp, C.c_int, C.c_int, C.c_int, _sz, _vp, _vp, C.c_int, C.c_int, _sz, _sz, C.c_float, C.c_float, C.c_int, _vp]),
    "savgol2d_gradient_batch_i16_route": (C.c_int, [C.c_int] * 3 + [_vp, C.c_int, C.c_int, C.c_int, _sz, _vp, _vp, C.c_int, C.c_int, _sz, _sz, C.c_float, C.c_float, C.c_int]),
    "savgol2d_gradient_batch_f32": (C.c_int, [C.c_int] * 3 + [_vp, C.c_int, C.c_int, C.c_int, _sz, _vp, _vp, C.c_int, _sz, _sz, C.c_float, C.c_float, C.c_int, _vp]),
    "savgol2d_hessian_batch_f32": (C.c_int, [C.c_int] * 3 + [_vp, C.c_int, C.c_int, C.c_int, _sz, _vp, _vp, _vp, C.c_int, _sz, _sz, C.c_float, C.c_float, C.c_int, _vp]),
    "savgol2d_laplacian_batch_f32": (C.c_int, [C.c_int] * 3 + [_vp, C.c_int, C.c_int, C.c_int, _sz, _vp, C.c_int, _sz, _sz, C.c_float, C.c_float, C.c_int, _vp]),
    # savgol_hip.h: 2-D row bands
    "savgol2d_rowband_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "savgol2d_apply_rowband_f32": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, _sz, _vp, _vp, C.c_int, _sz, _vp, C.c_int, _sz, _sz, C.c_int, C.c_int, _vp]),
    "savgol2d_apply_rowband_edges_f32": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, _sz, _vp, _vp, C.c_int, _sz, _vp, C.c_int, _sz, _sz, C.c_int, C.c_int, _vp]),
    "savgol2d_apply_rowband_edges_streams_f32": (C.c_int, [_F2, _vp, C.c_int, C.c_int, C.c_int, _sz, _vp, _vp, C.c_int, _sz, _vp, C.c_int, _sz, _sz, C.c_int, C.c_int, _vp, _vp]),
    # savgol_hip.h: bench utilities
    "savgol_hip_stream_copy": (C.c_int, [_vp, _vp, _sz, _vp]),
    "savgol_hip_stream_read": (C.c_int, [_vp, _sz, _vp, _vp]),
    "savgol_hip_synth_f32": (C.c_int, [_vp, _sz, _sz, _sz, _sz, C.c_uint64, _vp]),
    "savgol_hip_synth_f64": (C.c_int, [_vp, _sz, _sz, _sz, _sz, C.c_uint64, _vp]),
}

_lib = None


def lib():
    """The loaded C ABI.  Raises if libsavgol_hip.so was not built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {_HERE} -j8` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        try:                # if torch is around, let it load ITS HIP runtime first so both share one copy
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def last_error():
    return lib().savgol_hip_last_error().decode()


def device_count():
    return lib().savgol_hip_device_count()


def _addr(x):
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return int(x)


def _stream(stream):
    """None -> torch's current stream if torch has a GPU, else the default stream."""
    if stream is not None:
        return getattr(stream, "cuda_stream", stream)
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_stream().cuda_stream
    except Exception:
        pass
    return None


def _f(a):
    return a.ctypes.data_as(_fp)


def shard_range(total, world_size, rank):
    """Contiguous slice [lo, hi) of `total` independent units (channels, streams, images) owned by `rank`.

    The hot path has no exchange step, so multi-GPU = every rank filters its own slice; the first
    `total % world_size` ranks take one unit more."""
    if world_size < 1 or not (0 <= rank < world_size):
        raise ValueError("bad world_size / rank")
    q, r = divmod(total, world_size)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


class Filter:
    """RAII wrapper around savgol_create / savgol_destroy with the apply entry points as methods."""

    def __init__(self, half_window, poly_order, derivative=0, time_step=1.0, boundary=SAVGOL_BOUNDARY_POLYNOMIAL):
        cfg = SavgolConfig(half_window, poly_order, derivative, time_step, boundary)
        self.ptr = lib().savgol_create(C.byref(cfg))
        if not self.ptr:
            raise ValueError("savgol_create rejected the configuration")
        self.n = half_window
        self.ws = 2 * half_window + 1

    def close(self):
        if getattr(self, "ptr", None) and _lib is not None:      # (_lib is gone at interpreter shutdown)
            _lib.savgol_destroy(self.ptr)
        self.ptr = None

    __del__ = close

    # tables, as numpy copies
    @property
    def center_weights(self):
        return np.array(self.ptr.contents.center_weights[:self.ws], dtype=np.float32)

    @property
    def edge_weights(self):
        ew = self.ptr.contents.edge_weights
        return np.array([list(ew[e][:self.ws]) for e in range(self.n)], dtype=np.float32).reshape(self.n, self.ws)

    @property
    def dt_scale(self):
        return np.float32(self.ptr.contents.dt_scale)

    # ---- host-pointer drop-in calls (numpy in, numpy out) ----
    def apply(self, x, out=None):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x) if out is None else out
        rc = lib().savgol_apply(self.ptr, _f(x), _f(y), x.size)
        if rc != 0:
            raise RuntimeError(f"savgol_apply returned {rc}: {last_error()}")
        return y

    def apply_valid(self, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty(max(x.size - 2 * self.n, 1), np.float32)
        got = lib().savgol_apply_valid(self.ptr, _f(x), x.size, _f(y))
        return y[:got]

    def apply_strided(self, src, in_stride, in_offset, dst, out_stride, out_offset, count):
        return lib().savgol_apply_strided(self.ptr, src.ctypes.data, in_stride, in_offset,
                                          dst.ctypes.data, out_stride, out_offset, count)

    # ---- device-pointer batch calls (torch tensors or raw addresses) ----
    def apply_batch(self, d_in, d_out, channels, length, in_ld=None, out_ld=None, dtype="f32", valid=False, stream=None, flags=None, rel_tol=None,
                    out_dtype=None):
        """flags=None: the process-wide defaults (savgol_hip_set_option); an int: the *_ex entry point with exactly these SAVGOL_BATCH_* flags;
        rel_tol (fp64 only): savgol_apply[_valid]_batch_f64_tol -- the accuracy the caller accepts picks the kernel.
        dtype "f16" / "bf16": savgol_apply[_valid]_batch_h16 -- 16-bit rows in, out_dtype (None = the same type, or "f32") out, fp32 arithmetic;
        flags is that call's complete SAVGOL_BATCH_* word (None = 0); in_ld / out_ld count elements of their own buffer."""
        if dtype in ("f16", "bf16"):
            assert rel_tol is None
            name = f"savgol_apply_{'valid_' if valid else ''}batch_h16"
            rc = getattr(lib(), name)(self.ptr, _addr(d_in), _STORAGE[dtype], _addr(d_out), _STORAGE[dtype if out_dtype is None else out_dtype], channels, length,
                                      length if in_ld is None else in_ld, (length - 2 * self.n if valid else length) if out_ld is None else out_ld,
                                      0 if flags is None else flags, _stream(stream))
            if rc != 0:
                raise RuntimeError(f"{name} returned {rc}: {last_error()}")
            return
        assert out_dtype is None or out_dtype == dtype, "out_dtype belongs to the 16-bit storage types"
        assert rel_tol is None or (dtype == "f64" and flags is None)
        name = f"savgol_apply_{'valid_' if valid else ''}batch_{dtype}" + ("_tol" if rel_tol is not None else ("" if flags is None else "_ex"))
        args = [self.ptr, _addr(d_in), _addr(d_out), channels, length, length if in_ld is None else in_ld,
                (length - 2 * self.n if valid else length) if out_ld is None else out_ld]
        rc = getattr(lib(), name)(*args, *([float(rel_tol)] if rel_tol is not None else ([] if flags is None else [flags])), _stream(stream))
        if rc != 0:
            raise RuntimeError(f"{name} returned {rc}: {last_error()}")

    def apply_tensor(self, x, valid=False, stream=None, flags=None, out_dtype=None):
        """x: contiguous 2-D torch tensor [channels, length] (float32, float64, float16 or bfloat16) on the GPU.
        out_dtype (float16 / bfloat16 input only): None = the input's type, or torch.float32."""
        import torch
        names = {torch.float32: "f32", torch.float64: "f64", torch.float16: "f16", torch.bfloat16: "bf16"}
        if x.dtype not in names:
            raise TypeError(f"apply_tensor serves float32, float64, float16 and bfloat16 tensors, not {x.dtype}")
        dtype = names[x.dtype]
        if out_dtype is not None and out_dtype != x.dtype and not (dtype in ("f16", "bf16") and out_dtype == torch.float32):
            raise TypeError(f"apply_tensor: {x.dtype} -> {out_dtype} is not served")
        assert x.is_cuda and x.dim() == 2 and x.is_contiguous()
        ch, length = x.shape
        out_len = length - 2 * self.n if valid else length
        y = torch.empty((ch, out_len), dtype=x.dtype if out_dtype is None else out_dtype, device=x.device)
        self.apply_batch(x, y, ch, length, length, out_len, dtype=dtype, valid=valid, stream=stream, flags=flags,
                         out_dtype=None if out_dtype is None else names[out_dtype])
        return y

    def apply_batch_i16(self, d_in, d_out, channels, length, in_ld=None, out_ld=None, out_dtype="i16", valid=False, stream=None, flags=0):
        """savgol_apply[_valid]_batch_i16: int16 rows in, out_dtype "i16" or "f32" out, fp32 arithmetic; the fp32 narrow-tile call's bits on the widened
        input, for "i16" rounded to nearest even and saturated (NaN gives 0).  flags is the call's complete SAVGOL_BATCH_* word; in_ld / out_ld count
        elements of their own buffer."""
        types = {"i16": SAVGOL_HIP_I16, "f32": SAVGOL_HIP_F32}
        if out_dtype not in types:
            raise ValueError(f"apply_batch_i16: out_dtype {out_dtype!r} (\"i16\" or \"f32\")")
        name = f"savgol_apply_{'valid_' if valid else ''}batch_i16"
        rc = getattr(lib(), name)(self.ptr, _addr(d_in), _addr(d_out), types[out_dtype], channels, length, length if in_ld is None else in_ld,
                                  (length - 2 * self.n if valid else length) if out_ld is None else out_ld, flags, _stream(stream))
        if rc != 0:
            raise RuntimeError(f"{name} returned {rc}: {last_error()}")

    def apply_tensor_i16(self, x, valid=False, flags=0, out_dtype=None, stream=None):
        """x: contiguous 2-D torch.int16 tensor [channels, length] on the GPU.  out_dtype: None = int16, or torch.float32."""
        import torch
        if x.dtype != torch.int16:
            raise TypeError(f"apply_tensor_i16 serves int16 tensors, not {x.dtype}")
        if out_dtype not in (None, torch.int16, torch.float32):
            raise TypeError(f"apply_tensor_i16: {x.dtype} -> {out_dtype} is not served")
        assert x.is_cuda and x.dim() == 2 and x.is_contiguous()
        ch, length = x.shape
        out_len = length - 2 * self.n if valid else length
        y = torch.empty((ch, out_len), dtype=torch.int16 if out_dtype is None else out_dtype, device=x.device)
        self.apply_batch_i16(x, y, ch, length, length, out_len, out_dtype="f32" if out_dtype == torch.float32 else "i16", valid=valid, stream=stream, flags=flags)
        return y


def apply_multi_batch(filters, d_in, d_outs, channels, length, in_ld=None, out_ld=None, flags=0, valid=False, stream=None, dtype="f32", out_dtype=None):
    """savgol_apply[_valid]_multi_batch_f32: several Filters of one half window and boundary on one read of d_in (fp32 device memory).
    d_outs[k] receives filters[k]'s output, bit-identical to filters[k].apply_batch(..., flags=flags | SAVGOL_BATCH_PLAIN_SUMMATION).
    dtype "f16" / "bf16": savgol_apply[_valid]_multi_batch_h16 -- 16-bit rows in, every output of out_dtype (None = the same type, or "f32"); in_ld /
    out_ld count elements of their own buffer; d_outs[k] is bit-identical to filters[k].apply_batch(..., dtype=dtype, out_dtype=out_dtype,
    flags=flags | SAVGOL_BATCH_PLAIN_SUMMATION)."""
    count = len(filters)
    if len(d_outs) != count:
        raise ValueError("one output per filter")
    n = filters[0].n if count else 0
    fs = (_F * max(count, 1))(*[f.ptr for f in filters])
    outs = (_vp * max(count, 1))(*[_addr(o) for o in d_outs])
    in_ld = length if in_ld is None else in_ld
    out_ld = (length - 2 * n if valid else length) if out_ld is None else out_ld
    if dtype in ("f16", "bf16"):
        name = f"savgol_apply_{'valid_' if valid else ''}multi_batch_h16"
        rc = getattr(lib(), name)(fs, count, _addr(d_in), _STORAGE[dtype], outs, _STORAGE[dtype if out_dtype is None else out_dtype], channels, length, in_ld, out_ld,
                                  flags, _stream(stream))
    else:
        assert dtype == "f32" and out_dtype in (None, "f32"), "the multi-output call serves f32, f16 and bf16 rows; out_dtype belongs to the 16-bit storage types"
        name = f"savgol_apply_{'valid_' if valid else ''}multi_batch_f32"
        rc = getattr(lib(), name)(fs, count, _addr(d_in), outs, channels, length, in_ld, out_ld, flags, _stream(stream))
    if rc != 0:
        raise RuntimeError(f"{name} returned {rc}: {last_error()}")


def apply_multi_batch_i16(filters, d_in, d_outs, channels, length, in_ld=None, out_ld=None, out_dtype="i16", flags=0, valid=False, stream=None):
    """savgol_apply[_valid]_multi_batch_i16: several Filters of one half window and boundary on one read of d_in (int16 device memory), every output of
    out_dtype "i16" or "f32".  in_ld / out_ld count elements of their own buffer; d_outs[k] is bit-identical to filters[k].apply_batch_i16(...,
    out_dtype=out_dtype, flags=flags | SAVGOL_BATCH_PLAIN_SUMMATION)."""
    types = {"i16": SAVGOL_HIP_I16, "f32": SAVGOL_HIP_F32}
    if out_dtype not in types:
        raise ValueError(f"apply_multi_batch_i16: out_dtype {out_dtype!r} (\"i16\" or \"f32\")")
    count = len(filters)
    if len(d_outs) != count:
        raise ValueError("one output per filter")
    n = filters[0].n if count else 0
    fs = (_F * max(count, 1))(*[f.ptr for f in filters])
    outs = (_vp * max(count, 1))(*[_addr(o) for o in d_outs])
    name = f"savgol_apply_{'valid_' if valid else ''}multi_batch_i16"
    rc = getattr(lib(), name)(fs, count, _addr(d_in), outs, types[out_dtype], channels, length, length if in_ld is None else in_ld,
                              (length - 2 * n if valid else length) if out_ld is None else out_ld, flags, _stream(stream))
    if rc != 0:
        raise RuntimeError(f"{name} returned {rc}: {last_error()}")


def _field_jobs(jobs):
    return (SavgolFieldJob * max(len(jobs), 1))(*[SavgolFieldJob(f.ptr, in_offset, out_offset) for f, in_offset, out_offset in jobs])


def apply_strided_multi_batch(jobs, d_in, in_stride, in_channel_pitch, d_out, out_stride, out_channel_pitch, channels, count, flags=0, stream=None):
    """savgol_apply_strided_multi_batch_f32: several fields of an array of structs from one pass.  jobs: [(Filter, in_offset, out_offset)], byte offsets
    inside a record; job k filters the field at in_offset of the grid (d_in, in_stride, in_channel_pitch) into the field at out_offset of the grid
    (d_out, out_stride, out_channel_pitch).  Memory is left as the single strided calls in this order would leave it, bit for bit."""
    rc = lib().savgol_apply_strided_multi_batch_f32(_field_jobs(jobs), len(jobs), _addr(d_in), in_stride, in_channel_pitch, _addr(d_out), out_stride,
                                                    out_channel_pitch, channels, count, flags, _stream(stream))
    if rc != 0:
        raise RuntimeError(f"savgol_apply_strided_multi_batch_f32 returned {rc}: {last_error()}")


def apply_strided_multi_batch_route(jobs, d_in, in_stride, in_channel_pitch, d_out, out_stride, out_channel_pitch, channels, count, flags=0):
    """what the call above would do, without a device: the number of fused launches, 0 = len(jobs) single calls, -1 = refused (last_error() has the text)"""
    return lib().savgol_apply_strided_multi_batch_f32_route(_field_jobs(jobs), len(jobs), _addr(d_in), in_stride, in_channel_pitch, _addr(d_out), out_stride,
                                                            out_channel_pitch, channels, count, flags)


def apply_multi_tensor(filters, x, valid=False, flags=0, stream=None, out_dtype=None):
    """x: contiguous 2-D float32, float16 or bfloat16 torch tensor [channels, length] on the GPU; returns one tensor per filter (same order).
    out_dtype (float16 / bfloat16 input only): None = the input's type, or torch.float32."""
    import torch
    names = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
    if x.dtype not in names:
        raise TypeError(f"apply_multi_tensor serves float32, float16 and bfloat16 tensors, not {x.dtype}")
    dtype = names[x.dtype]
    if out_dtype is not None and out_dtype != x.dtype and not (dtype in ("f16", "bf16") and out_dtype == torch.float32):
        raise TypeError(f"apply_multi_tensor: {x.dtype} -> {out_dtype} is not served")
    assert x.is_cuda and x.dim() == 2 and x.is_contiguous()
    ch, length = x.shape
    out_len = length - 2 * filters[0].n if valid else length
    ys = [torch.empty((ch, out_len), dtype=x.dtype if out_dtype is None else out_dtype, device=x.device) for _ in filters]
    apply_multi_batch(filters, x, ys, ch, length, length, out_len, flags=flags, valid=valid, stream=stream, dtype=dtype,
                      out_dtype=None if out_dtype is None else names[out_dtype])
    return ys


def apply_multi_tensor_i16(filters, x, valid=False, flags=0, out_dtype=None, stream=None):
    """x: contiguous 2-D torch.int16 tensor [channels, length] on the GPU; returns one tensor per filter (same order).  out_dtype: None = int16, or
    torch.float32."""
    import torch
    if x.dtype != torch.int16:
        raise TypeError(f"apply_multi_tensor_i16 serves int16 tensors, not {x.dtype}")
    if out_dtype not in (None, torch.int16, torch.float32):
        raise TypeError(f"apply_multi_tensor_i16: {x.dtype} -> {out_dtype} is not served")
    assert x.is_cuda and x.dim() == 2 and x.is_contiguous()
    ch, length = x.shape
    out_len = length - 2 * filters[0].n if valid else length
    ys = [torch.empty((ch, out_len), dtype=torch.int16 if out_dtype is None else out_dtype, device=x.device) for _ in filters]
    apply_multi_batch_i16(filters, x, ys, ch, length, length, out_len, out_dtype="f32" if out_dtype == torch.float32 else "i16", flags=flags, valid=valid,
                          stream=stream)
    return ys


def synth(tensor, channel0=0, seed=0x5A17601A, stream=None):
    """Fill a contiguous [channels, length] GPU tensor with the SURVEY 8(d) synthetic workload."""
    import torch
    ch, length = tensor.shape
    fn = {torch.float32: lib().savgol_hip_synth_f32, torch.float64: lib().savgol_hip_synth_f64}[tensor.dtype]
    rc = fn(tensor.data_ptr(), channel0, ch, length, tensor.stride(0), seed, _stream(stream))
    if rc != 0:
        raise RuntimeError(f"savgol_hip_synth returned {rc}: {last_error()}")
    return tensor


class Stream:
    """savgol_stream_* on one host-side SavgolStream (the reference's streaming API, state in the POD)."""

    def __init__(self, half_window, poly_order, derivative=0, time_step=1.0):
        cfg = SavgolConfig(half_window, poly_order, derivative, time_step, 0)
        self.ptr = lib().savgol_stream_create(C.byref(cfg))
        if not self.ptr:
            raise ValueError("savgol_stream_create rejected the configuration")
        self.n = half_window

    def close(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.savgol_stream_destroy(self.ptr)
        self.ptr = None

    __del__ = close

    def push(self, x):
        ok = C.c_bool(False)
        y = lib().savgol_stream_push(self.ptr, float(x), C.byref(ok))
        return np.float32(y), bool(ok.value)

    def push_full(self, x, max_outputs=SAVGOL_MAX_HALF_WINDOW + 1):
        buf = np.zeros(max(max_outputs, 1), np.float32)
        c = lib().savgol_stream_push_full(self.ptr, float(x), _f(buf), max_outputs)
        return buf[:c].copy()

    def flush(self, max_count=SAVGOL_MAX_HALF_WINDOW):
        buf = np.zeros(max(max_count, 1), np.float32)
        c = lib().savgol_stream_flush(self.ptr, _f(buf), max_count)
        return c, buf[:max(c, 0)].copy()

    def flush_leading(self, max_count=SAVGOL_MAX_HALF_WINDOW):
        buf = np.zeros(max(max_count, 1), np.float32)
        c = lib().savgol_stream_flush_leading(self.ptr, _f(buf), max_count)
        return c, buf[:max(c, 0)].copy()

    @property
    def counters(self):
        s = self.ptr.contents
        return int(s.samples_received), int(s.samples_output), int(s.write_pos)


class StreamBank:
    """savgol_streambank_*: `streams` lock-step streams with their rings in HBM (torch tensors in/out)."""

    def __init__(self, streams, half_window, poly_order, derivative=0, time_step=1.0, fma=False):
        """fma=True: SAVGOL_STREAMBANK_FMA (fused multiply-adds: fast, not the reference's bits)."""
        cfg = SavgolConfig(half_window, poly_order, derivative, time_step, 0)
        self.ptr = lib().savgol_streambank_create_ex(C.byref(cfg), streams, SAVGOL_STREAMBANK_FMA if fma else 0)
        if not self.ptr:
            raise RuntimeError(f"savgol_streambank_create failed: {last_error()}")
        self.streams, self.n = streams, half_window

    def close(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.savgol_streambank_destroy(self.ptr)
        self.ptr = None

    __del__ = close

    def reset(self, stream=None):
        return lib().savgol_streambank_reset(self.ptr, _stream(stream))

    def push(self, samples, out, stream=None):
        return lib().savgol_streambank_push(self.ptr, _addr(samples), _addr(out), _stream(stream))

    def push_wait(self, samples, out, stream=None):
        """push + wait for the outputs through a stream-written completion word (savgol_streambank_push_wait)"""
        return lib().savgol_streambank_push_wait(self.ptr, _addr(samples), _addr(out), _stream(stream))

    def push_full(self, samples, out, max_rows, stream=None):
        return lib().savgol_streambank_push_full(self.ptr, _addr(samples), _addr(out), max_rows, _stream(stream))

    def push_block(self, samples, ticks, out, stream=None):
        return lib().savgol_streambank_push_block(self.ptr, _addr(samples), ticks, _addr(out), _stream(stream))

    def push_block_h16(self, samples, dtype, ticks, out, out_dtype=None, stream=None):
        """savgol_streambank_push_block_h16: `ticks` rows of fp16 / bf16 samples (dtype "f16" / "bf16"), outputs of out_dtype (None = the same type, or
        "f32"); the fp32 block push's results on the widened samples, rounded once to nearest even"""
        out_dtype = dtype if out_dtype is None else out_dtype
        if dtype not in _STORAGE or out_dtype not in _STORAGE:
            raise ValueError(f"push_block_h16: dtype {dtype!r} -> {out_dtype!r}")
        return lib().savgol_streambank_push_block_h16(self.ptr, _addr(samples), _STORAGE[dtype], ticks, _addr(out), _STORAGE[out_dtype], _stream(stream))

    def push_block_i16(self, samples, ticks, out, out_dtype="i16", stream=None):
        """savgol_streambank_push_block_i16: `ticks` rows of int16 samples, outputs of out_dtype ("i16" or "f32"); the fp32 block push's results on
        the widened samples, for "i16" converted once: rounded to nearest even, saturated to [-32768, 32767], NaN gives 0"""
        types = {"i16": SAVGOL_HIP_I16, "f32": SAVGOL_HIP_F32}
        if out_dtype not in types:
            raise ValueError(f"push_block_i16: out_dtype {out_dtype!r} (\"i16\" or \"f32\")")
        return lib().savgol_streambank_push_block_i16(self.ptr, _addr(samples), ticks, _addr(out), types[out_dtype], _stream(stream))

    def service_start(self, idle_ms=0):
        if lib().savgol_streambank_service_start(self.ptr, idle_ms) != 0:
            raise RuntimeError(last_error())

    def service_tick(self, samples, out):
        return lib().savgol_streambank_service_tick(self.ptr, _addr(samples), _addr(out))

    def service_stop(self):
        if lib().savgol_streambank_service_stop(self.ptr) != 0:
            raise RuntimeError(last_error())

    def flush(self, out, max_rows, stream=None):
        return lib().savgol_streambank_flush(self.ptr, _addr(out), max_rows, _stream(stream))

    def flush_leading(self, out, max_rows, stream=None):
        return lib().savgol_streambank_flush_leading(self.ptr, _addr(out), max_rows, _stream(stream))

    @property
    def counters(self):
        return (lib().savgol_streambank_samples_received(self.ptr), lib().savgol_streambank_samples_output(self.ptr))

    def save(self, stream=None):
        blob = np.zeros(lib().savgol_streambank_state_bytes(self.ptr), np.uint8)
        if lib().savgol_streambank_save(self.ptr, blob.ctypes.data, _stream(stream)) != 0:
            raise RuntimeError(last_error())
        return blob

    def load(self, blob, stream=None):
        if lib().savgol_streambank_load(self.ptr, blob.ctypes.data, _stream(stream)) != 0:
            raise RuntimeError(last_error())


def _multi_args(banks, outs):
    if len(banks) != len(outs):
        raise ValueError(f"push_block_multi: {len(banks)} banks, {len(outs)} outputs")
    return (C.c_void_p * len(banks))(*[getattr(b, "ptr", b) for b in banks]), (C.c_void_p * len(outs))(*[_addr(o) for o in outs])


def push_block_multi(banks, samples, ticks, outs, stream=None):
    """savgol_streambank_push_block_multi: up to four StreamBanks take the same block of samples, read from memory once; outs[k] is bank k's output
    block.  Returns the list of produced counts, one per bank (each the single savgol_streambank_push_block's return value); raises on a refusal."""
    b, o = _multi_args(banks, outs)
    produced = (C.c_int * max(len(banks), 1))()
    if lib().savgol_streambank_push_block_multi(b, len(banks), _addr(samples), ticks, o, produced, _stream(stream)) < 0:
        raise RuntimeError(last_error())
    return list(produced)[:len(banks)]


def push_block_multi_route(banks, samples, ticks, outs):
    """the number of fused launches push_block_multi would make on these arguments (0 = one single block push per bank), -1 on a refusal; enqueues nothing"""
    b, o = _multi_args(banks, outs)
    return lib().savgol_streambank_push_block_multi_route(b, len(banks), _addr(samples), ticks, o)


def _multi_h16_types(dtype, out_dtype):
    out_dtype = dtype if out_dtype is None else out_dtype
    if dtype not in _STORAGE or out_dtype not in _STORAGE:
        raise ValueError(f"push_block_multi_h16: dtype {dtype!r} -> {out_dtype!r}")
    return _STORAGE[dtype], _STORAGE[out_dtype]


def push_block_multi_h16(banks, samples, dtype, ticks, outs, out_dtype=None, stream=None):
    """savgol_streambank_push_block_multi_h16: up to four StreamBanks take the same block of fp16 / bf16 samples (dtype "f16" / "bf16"), read from memory
    once; outs[k] is bank k's output block of out_dtype (None = the same type, or "f32").  Returns the list of produced counts, one per bank (each the
    single savgol_streambank_push_block_h16's return value); raises on a refusal."""
    b, o = _multi_args(banks, outs)
    it, ot = _multi_h16_types(dtype, out_dtype)
    produced = (C.c_int * max(len(banks), 1))()
    if lib().savgol_streambank_push_block_multi_h16(b, len(banks), _addr(samples), it, ticks, o, ot, produced, _stream(stream)) < 0:
        raise RuntimeError(last_error())
    return list(produced)[:len(banks)]


def push_block_multi_h16_route(banks, samples, dtype, ticks, outs, out_dtype=None):
    """the number of fused launches push_block_multi_h16 would make on these arguments (0 = one single 16-bit block push per bank), -1 on a refusal;
    enqueues nothing"""
    b, o = _multi_args(banks, outs)
    it, ot = _multi_h16_types(dtype, out_dtype)
    return lib().savgol_streambank_push_block_multi_h16_route(b, len(banks), _addr(samples), it, ticks, o, ot)


def _multi_i16_type(out_dtype):
    types = {"i16": SAVGOL_HIP_I16, "f32": SAVGOL_HIP_F32}
    if out_dtype not in types:
        raise ValueError(f"push_block_multi_i16: out_dtype {out_dtype!r} (\"i16\" or \"f32\")")
    return types[out_dtype]


def push_block_multi_i16(banks, samples, ticks, outs, out_dtype="i16", stream=None):
    """savgol_streambank_push_block_multi_i16: up to four StreamBanks take the same block of int16 samples, read from memory once; outs[k] is bank k's
    output block of out_dtype ("i16" or "f32").  Returns the list of produced counts, one per bank (each the single savgol_streambank_push_block_i16's
    return value); raises on a refusal."""
    b, o = _multi_args(banks, outs)
    ot = _multi_i16_type(out_dtype)
    produced = (C.c_int * max(len(banks), 1))()
    if lib().savgol_streambank_push_block_multi_i16(b, len(banks), _addr(samples), ticks, o, ot, produced, _stream(stream)) < 0:
        raise RuntimeError(last_error())
    return list(produced)[:len(banks)]


def push_block_multi_i16_route(banks, samples, ticks, outs, out_dtype="i16"):
    """the number of fused launches push_block_multi_i16 would make on these arguments (0 = one single int16 block push per bank), -1 on a refusal;
    enqueues nothing"""
    b, o = _multi_args(banks, outs)
    return lib().savgol_streambank_push_block_multi_i16_route(b, len(banks), _addr(samples), ticks, o, _multi_i16_type(out_dtype))


class Filter2D:
    """savgol2d_create / savgol2d_destroy + the apply entry points."""

    def __init__(self, nx, ny, order, dx=0, dy=0, delta_x=1.0, delta_y=1.0):
        cfg = Savgol2DConfig(nx, ny, order, dx, dy, delta_x, delta_y)
        self.ptr = lib().savgol2d_create(C.byref(cfg))
        if not self.ptr:
            raise ValueError("savgol2d_create rejected the configuration")
        self.nx, self.ny = nx, ny

    def close(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.savgol2d_destroy(self.ptr)
        self.ptr = None

    __del__ = close

    @property
    def weights(self):
        f = self.ptr.contents
        return np.array(f.weights[:f.window_area], dtype=np.float32).reshape(f.window_height, f.window_width)

    @property
    def scale(self):
        return np.float32(self.ptr.contents.scale)

    def apply(self, img, cols=None, boundary=SAVGOL2D_BOUNDARY_VALID, out=None):
        """img: 2-D fp32 numpy array, row pitch = img.shape[1]; returns a same-shape frame (copy of `out` or zeros)."""
        img = np.ascontiguousarray(img, np.float32)
        rows, stride = img.shape
        cols = stride if cols is None else cols
        o = np.array(out, np.float32, copy=True) if out is not None else np.zeros_like(img)
        rc = lib().savgol2d_apply(self.ptr, _f(img), rows, cols, stride, _f(o), stride, boundary)
        if rc != 0:
            raise RuntimeError(f"savgol2d_apply returned {rc}: {last_error()}")
        return o

    def apply_valid(self, img, cols=None):
        img = np.ascontiguousarray(img, np.float32)
        rows, stride = img.shape
        cols = stride if cols is None else cols
        o = np.zeros((rows - 2 * self.ny, cols - 2 * self.nx), np.float32)
        rc = lib().savgol2d_apply_valid(self.ptr, _f(img), rows, cols, stride, _f(o), o.shape[1])
        if rc != 0:
            raise RuntimeError(f"savgol2d_apply_valid returned {rc}: {last_error()}")
        return o

    def apply_batch(self, d_in, d_out, rows, cols, images, in_stride=None, out_stride=None, in_pitch=None, out_pitch=None,
                    boundary=SAVGOL2D_BOUNDARY_VALID, method=0, stream=None):
        in_stride = cols if in_stride is None else in_stride
        out_stride = cols if out_stride is None else out_stride
        rc = lib().savgol2d_apply_batch_f32(self.ptr, _addr(d_in), rows, cols, in_stride,
                                            rows * in_stride if in_pitch is None else in_pitch, _addr(d_out), out_stride,
                                            rows * out_stride if out_pitch is None else out_pitch, images, boundary, method,
                                            _stream(stream))
        if rc != 0:
            raise RuntimeError(f"savgol2d_apply_batch_f32 returned {rc}: {last_error()}")

    def apply_batch_h16(self, d_in, dtype, d_out, rows, cols, images, out_dtype=None, in_stride=None, out_stride=None, in_pitch=None, out_pitch=None,
                        boundary=SAVGOL2D_BOUNDARY_VALID, method=0, stream=None):
        """savgol2d_apply_batch_h16: frames of fp16 / bf16 pixels (dtype "f16" / "bf16"), outputs of out_dtype (None = the same type, or "f32"), the fp32
        call's arithmetic in between; strides and pitches count elements of their own buffer."""
        out_dtype = dtype if out_dtype is None else out_dtype
        if dtype not in ("f16", "bf16") or out_dtype not in (dtype, "f32"):
            raise ValueError(f"apply_batch_h16: dtype {dtype!r} -> {out_dtype!r}")
        in_stride = cols if in_stride is None else in_stride
        out_stride = cols if out_stride is None else out_stride
        rc = lib().savgol2d_apply_batch_h16(self.ptr, _addr(d_in), _STORAGE[dtype], rows, cols, in_stride,
                                            rows * in_stride if in_pitch is None else in_pitch, _addr(d_out), _STORAGE[out_dtype], out_stride,
                                            rows * out_stride if out_pitch is None else out_pitch, images, boundary, method, _stream(stream))
        if rc != 0:
            raise RuntimeError(f"savgol2d_apply_batch_h16 returned {rc}: {last_error()}")

    def _i16_args(self, who, d_in, d_out, rows, cols, images, out_dtype, in_stride, out_stride, in_pitch, out_pitch, boundary, method):
        types = {"i16": SAVGOL_HIP_I16, "f32": SAVGOL_HIP_F32}
        if out_dtype not in types:
            raise ValueError(f"{who}: out_dtype {out_dtype!r} (\"i16\" or \"f32\")")
        in_stride = cols if in_stride is None else in_stride
        out_stride = cols if out_stride is None else out_stride
        return (self.ptr, _addr(d_in), rows, cols, in_stride, rows * in_stride if in_pitch is None else in_pitch, _addr(d_out), types[out_dtype], out_stride,
                rows * out_stride if out_pitch is None else out_pitch, images, boundary, method)

    def apply_batch_i16(self, d_in, d_out, rows, cols, images, out_dtype="i16", in_stride=None, out_stride=None, in_pitch=None, out_pitch=None,
                        boundary=SAVGOL2D_BOUNDARY_VALID, method=0, stream=None):
        """savgol2d_apply_batch_i16: frames of int16 pixels, outputs of out_dtype ("i16" or "f32"), the fp32 call's arithmetic in between; for "i16" the fp32
        call's pixel rounded to nearest even and saturated (NaN gives 0).  Strides and pitches count elements of their own buffer."""
        args = self._i16_args("apply_batch_i16", d_in, d_out, rows, cols, images, out_dtype, in_stride, out_stride, in_pitch, out_pitch, boundary, method)
        rc = lib().savgol2d_apply_batch_i16(*args, _stream(stream))
        if rc != 0:
            raise RuntimeError(f"savgol2d_apply_batch_i16 returned {rc}: {last_error()}")

    def apply_batch_i16_route(self, d_in, d_out, rows, cols, images, out_dtype="i16", in_stride=None, out_stride=None, in_pitch=None, out_pitch=None,
                              boundary=SAVGOL2D_BOUNDARY_VALID, method=0):
        """the route apply_batch_i16 would take on these arguments, touching no device: 1 = the int16 tiles, 0 = staged through fp32 scratch (or no images),
        -1 = the call would be refused (last_error() has the text)"""
        return lib().savgol2d_apply_batch_i16_route(*self._i16_args("apply_batch_i16_route", d_in, d_out, rows, cols, images, out_dtype, in_stride, out_stride,
                                                                    in_pitch, out_pitch, boundary, method))


def _gradient_i16_args(who, nx, ny, order, d_in, d_gx, d_gy, rows, cols, images, out_dtype, in_stride, out_stride, in_pitch, out_pitch, delta_x, delta_y, boundary):
    types = {"i16": SAVGOL_HIP_I16, "f32": SAVGOL_HIP_F32}
    if out_dtype not in types:
        raise ValueError(f"{who}: out_dtype {out_dtype!r} (\"i16\" or \"f32\")")
    in_stride = cols if in_stride is None else in_stride
    out_stride = cols if out_stride is None else out_stride
    return (nx, ny, order, _addr(d_in), rows, cols, in_stride, rows * in_stride if in_pitch is None else in_pitch, _addr(d_gx), _addr(d_gy), types[out_dtype], out_stride,
            rows * out_stride if out_pitch is None else out_pitch, images, delta_x, delta_y, boundary)


def gradient_batch_i16(nx, ny, order, d_in, d_gx, d_gy, rows, cols, images, out_dtype="i16", in_stride=None, out_stride=None, in_pitch=None, out_pitch=None,
                       delta_x=1.0, delta_y=1.0, boundary=SAVGOL2D_BOUNDARY_VALID, stream=None):
    """savgol2d_gradient_batch_i16: frames of int16 pixels, gx and gy of out_dtype ("i16" or "f32"; either may be None), the fp32 gradient call's arithmetic
    in between; for "i16" the fp32 call's pixel rounded to nearest even and saturated (NaN gives 0).  Strides and pitches count elements of their own buffer."""
    args = _gradient_i16_args("gradient_batch_i16", nx, ny, order, d_in, d_gx, d_gy, rows, cols, images, out_dtype, in_stride, out_stride, in_pitch, out_pitch,
                              delta_x, delta_y, boundary)
    rc = lib().savgol2d_gradient_batch_i16(*args, _stream(stream))
    if rc != 0:
        raise RuntimeError(f"savgol2d_gradient_batch_i16 returned {rc}: {last_error()}")


def gradient_batch_i16_route(nx, ny, order, d_in, d_gx, d_gy, rows, cols, images, out_dtype="i16", in_stride=None, out_stride=None, in_pitch=None, out_pitch=None,
                             delta_x=1.0, delta_y=1.0, boundary=SAVGOL2D_BOUNDARY_VALID):
    """the route gradient_batch_i16 would take on these arguments, touching no device: 1 = the int16 kernels (direct), 0 = staged through fp32 scratch (or
    nothing to do), -1 = the call would be refused (last_error() has the text)"""
    return lib().savgol2d_gradient_batch_i16_route(*_gradient_i16_args("gradient_batch_i16_route", nx, ny, order, d_in, d_gx, d_gy, rows, cols, images, out_dtype,
                                                                      in_stride, out_stride, in_pitch, out_pitch, delta_x, delta_y, boundary))
