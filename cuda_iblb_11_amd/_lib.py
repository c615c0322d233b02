"""ctypes binding of include/iblb.h (the C ABI of libiblb.so).

The shared library is built in-tree (``make`` -> cuda_iblb_11_amd/lib/libiblb.so).  There is
no CPU fallback: if the library is missing, or no HIP device is visible, every compute
entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
# IBLB_LIB: another build of the same library (A/B measurements of kernel builds only)
LIB_PATH = os.environ.get("IBLB_LIB") or os.path.join(_HERE, "lib", "libiblb.so")
HEADER = os.path.join(REPO, "include", "iblb.h")

IBLB_OK = 0
IBLB_ERR_ARG = -1
IBLB_ERR_HIP = -2
IBLB_ERR_STATE = -3
IBLB_ERR_COMM = -4
IBLB_ERR_NOMEM = -5
IBLB_ERR_UNSUPPORTED = -6
IBLB_ERR_NODEVICE = -7
PREC_F64 = 0
PREC_F32 = 1
UNIQUE_ID_BYTES = 128

_ERRNAMES = {
    IBLB_ERR_ARG: "IBLB_ERR_ARG", IBLB_ERR_HIP: "IBLB_ERR_HIP", IBLB_ERR_STATE: "IBLB_ERR_STATE",
    IBLB_ERR_COMM: "IBLB_ERR_COMM", IBLB_ERR_NOMEM: "IBLB_ERR_NOMEM",
    IBLB_ERR_UNSUPPORTED: "IBLB_ERR_UNSUPPORTED", IBLB_ERR_NODEVICE: "IBLB_ERR_NODEVICE",
}


class IblbError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_ERRNAMES.get(code, code)}: {msg}")
        self.code = code


class Config(C.Structure):
    """struct iblb_config (include/iblb.h)."""
    _fields_ = [
        ("nx", C.c_int), ("ny", C.c_int),
        ("tau", C.c_double), ("tau2", C.c_double),
        ("precision", C.c_int),
        ("body_force", C.c_double * 2),
        ("flux_norm", C.c_double),
        ("flux_column", C.c_int),
        ("device", C.c_int),
        ("x_begin", C.c_int), ("x_count", C.c_int),
        ("max_points", C.c_int),
    ]


class Timing(C.Structure):
    """struct iblb_timing (include/iblb.h)."""
    _fields_ = [
        ("steps", C.c_longlong), ("fused_launches", C.c_longlong),
        ("fused_ms", C.c_double), ("ib_ms", C.c_double), ("halo_ms", C.c_double),
        ("fused_bytes", C.c_double), ("cells", C.c_longlong), ("fused_cells", C.c_longlong),
        ("sweep_launches", C.c_longlong), ("sweep_ms", C.c_double), ("sweep_cells", C.c_longlong),
        ("sweepk_launches", C.c_longlong), ("sweepk_ms", C.c_double), ("sweepk_cells", C.c_longlong), ("sweepk_depth", C.c_longlong),
        ("band_cycles", C.c_longlong), ("band_merged_cycles", C.c_longlong), ("band_par_cycles", C.c_longlong),
        ("deep_launches", C.c_longlong), ("deep_iterations", C.c_longlong),
        ("dev_wait_launches", C.c_longlong),
        ("deep_mode", C.c_longlong), ("deep_vs", C.c_longlong), ("deep_waves_per_simd", C.c_longlong),
        ("deep_vgprs", C.c_longlong),
    ]


class Cilia(C.Structure):
    """struct iblb_cilia (include/iblb.h)."""
    _fields_ = [("c_num", C.c_int), ("c_space", C.c_double), ("T", C.c_int), ("p_step", C.c_int)]


class Window(C.Structure):
    """struct iblb_window (include/iblb.h): the global cells (x0 + i*sx, y0 + j*sy), i < nx, j < ny."""
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("sx", C.c_int), ("sy", C.c_int)]


# the fluid's IBLB_FIELD_* bits of iblb_get_fields, in ascending bit order (the order of the output planes)
FIELDS = {"rho": 1, "ux": 2, "uy": 4, "vort": 8, "sxx": 16, "sxy": 32, "syy": 64}
# the passive scalar's fields (IBLB_FIELD_C, _CUX, _CUY): every reader takes them once a scalar is set
SCALAR_FIELDS = {"c": 4096, "cux": 8192, "cuy": 16384}
# what iblb_get_fields, iblb_sample_points and iblb_set_average accept, in ascending bit order
READ_FIELDS = {**FIELDS, **SCALAR_FIELDS}
# what iblb_reduce_fields accepts: those and the reduce-only IBLB_QTY_* bits, in ascending bit order
QUANTITIES = {**FIELDS, "momx": 128, "momy": 256, "ke": 512, "usq": 1024, **SCALAR_FIELDS}
# flags of iblb_set_average
AVG_SQ = 1
AVG_UXUY = 2
# flag of iblb_set_history: the positions are the context's tracers
HIST_TRACERS = 1
# wall kinds of iblb_set_scalar
SCALAR_WALL_NOFLUX = 0
SCALAR_WALL_VALUE = 1
# wall kinds and statuses of iblb_set_tracer_model
TRACER_WALLS = {"clamp": 0, "reflect": 1, "absorb": 2}
TRACER_ALIVE = 0
TRACER_AT_BOTTOM = 1
TRACER_AT_TOP = 2


class TracerModel(C.Structure):
    """struct iblb_tracer_model (include/iblb.h)."""
    _fields_ = [("diffusivity", C.c_double), ("drift", C.c_double * 2), ("wall", C.c_int * 2), ("seed", C.c_ulonglong)]


class Scalar(C.Structure):
    """struct iblb_scalar (include/iblb.h)."""
    _fields_ = [("tau", C.c_double), ("stride", C.c_int), ("wall_kind", C.c_int * 2), ("wall_value", C.c_double * 2)]


class ScalarSource(C.Structure):
    """struct iblb_scalar_source (include/iblb.h)."""
    _fields_ = [("source", C.c_void_p), ("decay", C.c_double), ("wall_flux", C.c_void_p * 2),
                ("wall_value", C.c_void_p * 2)]


# the `present` bits of iblb_scalar_source_info
SCALAR_SOURCE_SET = 1
SCALAR_SOURCE_FIELD = 2
SCALAR_SOURCE_WALL_FLUX = (4, 8)
SCALAR_SOURCE_WALL_VALUE = (16, 32)


class ScalarUptake(C.Structure):
    """struct iblb_scalar_uptake (include/iblb.h)."""
    _fields_ = [("rate", C.c_void_p * 2)]


# the `present` bits of iblb_scalar_uptake_info
SCALAR_UPTAKE_SET = 1
SCALAR_UPTAKE_RATE = (2, 4)

# end kinds of iblb_set_scalar_ends
SCALAR_END_NOFLUX = 0
SCALAR_END_VALUE = 1
SCALAR_END_OUTFLOW = 2
SCALAR_END_KINDS = {"noflux": SCALAR_END_NOFLUX, "value": SCALAR_END_VALUE, "outflow": SCALAR_END_OUTFLOW}


class ScalarEnds(C.Structure):
    """struct iblb_scalar_ends (include/iblb.h)."""
    _fields_ = [("kind", C.c_int * 2), ("value", C.c_double * 2), ("profile", C.c_void_p * 2)]


# the `present` bits of iblb_scalar_ends_info
SCALAR_ENDS_SET = 1
SCALAR_ENDS_PROFILE = (2, 4)


class ScalarGauges(C.Structure):
    """struct iblb_scalar_gauges (include/iblb.h)."""
    _fields_ = [("n_stations", C.c_int), ("station", C.c_void_p), ("n_levels", C.c_int), ("level", C.c_void_p)]


# the observers of iblb_save_checkpoint_ex / iblb_checkpoint_info (IBLB_CKPT_*)
CKPT_SCALAR = 1
CKPT_TRACERS = 2
CKPT_AVERAGE = 4
OBSERVERS = 7


class FieldStats(C.Structure):
    """struct iblb_field_stats (include/iblb.h)."""
    _fields_ = [
        ("count", C.c_longlong), ("nonfinite", C.c_longlong),
        ("sum", C.c_double), ("sum_sq", C.c_double),
        ("min", C.c_double), ("max", C.c_double),
        ("min_i", C.c_int), ("min_j", C.c_int), ("max_i", C.c_int), ("max_j", C.c_int),
    ]


_vp = C.c_void_p
_SIGS = {
    # (1) reference-shaped kernels: device pointers + stream
    "iblb_equilibrium": ([_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_double, _vp], C.c_int),
    "iblb_collision": ([_vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _vp], C.c_int),
    "iblb_streaming": ([_vp, _vp, C.c_int, C.c_int, _vp], C.c_int),
    "iblb_macro": ([_vp, _vp, _vp, C.c_int, C.c_int, _vp], C.c_int),
    "iblb_interpolate": ([_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp], C.c_int),
    "iblb_spread": ([_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp], C.c_int),
    "iblb_spread_ex": ([_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int,
                        C.c_double, _vp], C.c_int),
    "iblb_delta": ([C.c_int, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "iblb_define_filament": ([C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, _vp, _vp, _vp, _vp], C.c_int),
    "iblb_boundary_check": ([C.c_double, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp], C.c_int),
    # (2) context API
    "iblb_config_default": ([C.POINTER(Config)], C.c_int),
    "iblb_create": ([C.POINTER(Config), C.POINTER(_vp)], C.c_int),
    "iblb_destroy": ([_vp], None),
    "iblb_last_error": ([_vp], C.c_char_p),
    "iblb_version": ([], C.c_char_p),
    "iblb_abi_version": ([], C.c_int),
    "iblb_device_count": ([C.POINTER(C.c_int)], C.c_int),
    "iblb_set_state": ([_vp, _vp, _vp, _vp, _vp], C.c_int),
    "iblb_set_lagrangian": ([_vp, C.c_int, _vp, _vp, _vp], C.c_int),
    "iblb_set_lagrangian_steps": ([_vp, C.c_int, C.c_int, _vp, _vp, _vp], C.c_int),
    "iblb_set_cilia": ([_vp, C.POINTER(Cilia)], C.c_int),
    "iblb_get_lagrangian": ([_vp, _vp, _vp, _vp], C.c_int),
    "iblb_step": ([_vp, C.c_int], C.c_int),
    "iblb_get_macro": ([_vp, _vp, _vp], C.c_int),
    "iblb_get_populations": ([_vp, _vp], C.c_int),
    "iblb_get_force": ([_vp, _vp], C.c_int),
    "iblb_get_lagrangian_force": ([_vp, _vp], C.c_int),
    "iblb_get_flux": ([_vp, C.POINTER(C.c_double)], C.c_int),
    "iblb_get_step": ([_vp, C.POINTER(C.c_longlong)], C.c_int),
    "iblb_count_nonfinite": ([_vp, C.POINTER(C.c_longlong)], C.c_int),
    "iblb_window_local": ([_vp, C.POINTER(Window), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "iblb_get_fields": ([_vp, C.POINTER(Window), C.c_uint, _vp], C.c_int),
    "iblb_reduce_fields": ([_vp, C.POINTER(Window), C.c_uint, C.POINTER(FieldStats), _vp, _vp], C.c_int),
    "iblb_sample_points": ([_vp, C.c_int, _vp, _vp, C.c_uint, _vp], C.c_int),
    "iblb_set_tracers": ([_vp, C.c_longlong, _vp, _vp, C.c_int], C.c_int),
    "iblb_get_tracers": ([_vp, _vp, _vp, _vp], C.c_int),
    "iblb_tracer_count": ([_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong)], C.c_int),
    "iblb_set_tracer_model": ([_vp, C.POINTER(TracerModel), _vp, _vp], C.c_int),
    "iblb_tracer_model_info": ([_vp, C.POINTER(TracerModel), C.POINTER(C.c_int), C.POINTER(C.c_longlong)], C.c_int),
    "iblb_get_tracer_fates": ([_vp, _vp, _vp], C.c_int),
    "iblb_get_tracer_deposits": ([_vp, _vp, _vp], C.c_int),
    "iblb_set_average": ([_vp, C.POINTER(Window), C.c_uint, C.c_int, C.c_int, C.c_uint], C.c_int),
    "iblb_reset_average": ([_vp], C.c_int),
    "iblb_get_average": ([_vp, C.c_int, _vp, _vp, _vp, C.POINTER(C.c_longlong)], C.c_int),
    "iblb_average_info": ([_vp, C.POINTER(Window), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_int),
                           C.POINTER(C.c_uint), C.POINTER(C.c_longlong)], C.c_int),
    "iblb_set_history": ([_vp, C.c_longlong, _vp, _vp, C.c_uint, C.c_int, C.c_longlong, C.c_uint], C.c_int),
    "iblb_get_history": ([_vp, C.c_longlong, C.c_longlong, _vp, _vp], C.c_int),
    "iblb_get_history_stats": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "iblb_get_history_points": ([_vp, _vp, _vp], C.c_int),
    "iblb_reset_history": ([_vp], C.c_int),
    "iblb_history_info": ([_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_uint), C.POINTER(C.c_int),
                           C.POINTER(C.c_longlong), C.POINTER(C.c_uint), C.POINTER(C.c_longlong)], C.c_int),
    "iblb_set_scalar": ([_vp, C.POINTER(Scalar), _vp, _vp], C.c_int),
    "iblb_get_scalar": ([_vp, C.POINTER(Window), _vp], C.c_int),
    "iblb_get_scalar_populations": ([_vp, _vp], C.c_int),
    "iblb_scalar_info": ([_vp, C.POINTER(Scalar), C.POINTER(C.c_longlong)], C.c_int),
    "iblb_get_scalar_wall_flux": ([_vp, _vp, _vp], C.c_int),
    "iblb_set_scalar_source": ([_vp, C.POINTER(ScalarSource)], C.c_int),
    "iblb_scalar_source_info": ([_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint)], C.c_int),
    "iblb_get_scalar_source": ([_vp, _vp], C.c_int),
    "iblb_set_scalar_uptake": ([_vp, C.POINTER(ScalarUptake)], C.c_int),
    "iblb_get_scalar_uptake": ([_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_longlong)], C.c_int),
    "iblb_reset_scalar_uptake": ([_vp], C.c_int),
    "iblb_scalar_uptake_info": ([_vp, C.POINTER(C.c_uint), C.POINTER(C.c_longlong)], C.c_int),
    "iblb_set_scalar_ends": ([_vp, C.POINTER(ScalarEnds)], C.c_int),
    "iblb_get_scalar_ends": ([_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_longlong)], C.c_int),
    "iblb_reset_scalar_ends": ([_vp], C.c_int),
    "iblb_scalar_ends_info": ([_vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint),
                               C.POINTER(C.c_longlong)], C.c_int),
    "iblb_set_scalar_gauges": ([_vp, C.POINTER(ScalarGauges)], C.c_int),
    "iblb_get_scalar_gauges": ([_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_longlong)], C.c_int),
    "iblb_reset_scalar_gauges": ([_vp], C.c_int),
    "iblb_scalar_gauges_info": ([_vp, C.POINTER(C.c_int), _vp, C.POINTER(C.c_int), _vp, C.POINTER(C.c_longlong)],
                                C.c_int),
    "iblb_set_profiling": ([_vp, C.c_int], C.c_int),
    "iblb_get_timing": ([_vp, C.POINTER(Timing), C.c_int], C.c_int),
    "iblb_get_timing_ex": ([_vp, C.POINTER(Timing), C.c_ulong, C.c_int], C.c_int),
    "iblb_deep_force_build": ([_vp], C.c_int),
    "iblb_get_stream": ([_vp, C.POINTER(_vp)], C.c_int),
    "iblb_synchronize": ([_vp], C.c_int),
    "iblb_link_local": ([C.POINTER(_vp), C.c_int], C.c_int),
    "iblb_group_step": ([C.POINTER(_vp), C.c_int, C.c_int], C.c_int),
    "iblb_rccl_unique_id": ([C.c_char_p], C.c_int),
    "iblb_attach_rccl": ([_vp, C.c_char_p, C.c_int, C.c_int], C.c_int),
    "iblb_set_wait_timeout": ([_vp, C.c_double], C.c_int),
    "iblb_gather_macro": ([_vp, C.c_int, _vp, _vp], C.c_int),
    "iblb_save_checkpoint": ([_vp, C.c_char_p], C.c_int),
    "iblb_load_checkpoint": ([_vp, C.c_char_p], C.c_int),
    "iblb_save_checkpoint_ex": ([_vp, C.c_char_p, C.c_uint], C.c_int),
    "iblb_checkpoint_info": ([C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(C.c_uint)], C.c_int),
}

_lib = None


def header_functions() -> list[str]:
    """Names of every function declared in include/iblb.h."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(iblb_[a-z_]+)\s*\(", text)))


def configure(lib: C.CDLL) -> C.CDLL:
    """Attach the include/iblb.h signatures to a loaded library."""
    for name, (args, res) in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


def load_from(path: str) -> C.CDLL:
    """Load another build of the C ABI (e.g. the mock-RCCL test build) without torch."""
    return configure(C.CDLL(path))


def load() -> C.CDLL:
    """Load libiblb.so (raises if it was not built; there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `make` (hipcc, gfx950); there is no CPU fallback")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 / librccl.so.1.  If torch
    # is importable, load it first so libiblb binds to the same runtime (same SONAMEs) instead of
    # a second copy from /opt/rocm, which would leave torch without devices.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    _lib = configure(C.CDLL(LIB_PATH))
    return _lib


def check(rc: int, ctx=None, lib: C.CDLL | None = None) -> None:
    if rc != IBLB_OK:
        msg = (lib or load()).iblb_last_error(ctx)
        raise IblbError(rc, msg.decode() if msg else "")


def device_count() -> int:
    n = C.c_int(0)
    load().iblb_device_count(C.byref(n))
    return n.value
