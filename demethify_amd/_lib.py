"""ctypes binding of libdemethify_hip.so (C-ABI declared in include/demethify_hip.h).

The product path has no CPU fallback: if the shared library is missing or no gfx950 device
is visible, every solver call raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "libdemethify_hip.so"

DMF_OK = 0
DMF_PTR_DEVICE = 1
DMF_INIT_IN_UNIT_RANGE = 4
DMF_SELECT_COUNTS_F32_EXACT, DMF_SELECT_PURITY, DMF_SELECT_ALPHA_OUTSIDE_UNIT, DMF_SELECT_V_UNALIGNED = 1, 2, 4, 8
DMF_SELECT_X16 = 16
DMF_SELECT_COUNTS_BYTE, DMF_SELECT_NO_ROWPASS_PAIR, DMF_SELECT_NO_ROWPASS_DEFER_C, DMF_SELECT_NO_ROWPASS_BYTES = 32, 64, 128, 256
DMF_COUNTS_F64 = 2
DMF_WLS_TARGET_V, DMF_WLS_TARGET_DV = 0, 1
DMF_WLS_F64_ARRAYS = 8
DMF_ERR_BAD_ARG, DMF_ERR_NONFINITE, DMF_ERR_UNSUPPORTED = 1, 4, 5
DMF_ERR_BAD_SHAPE = 2
DMF_GRAM_INTEGER, DMF_GRAM_FP64, DMF_GRAM_LAST = 0, 1, 2
DMF_ROUTE_SOLVER, DMF_ROUTE_UPDATE_U = 0, 1
# dmf_solver_momentum_state's scalars, in order (DMF_MOMENTUM_SCALARS of them; the last five are integers)
MOMENTUM_SCALARS = ("a1", "a2", "l_w", "l_w_prev", "l_h", "l_h_prev", "dsq", "rt_norm2", "u_norm2", "cf", "cf_prev",
                    "iters", "done", "arrive", "mom_n", "mom_i")
# dmf_problem_report's integers and doubles, in order (DMF_REPORT_INTS / DMF_REPORT_DBLS of them)
REPORT_INTS = ("N", "S", "n_c", "ND", "SD", "N16", "plane_stride", "has_D16", "has_X16", "has_W16", "has_Dt8", "has_mask_bits",
               "rtp_width", "rtp_borrows_rt", "n_test", "d_f32_exact")
REPORT_DBLS = ("kDsq", "kRtSumsq", "kDmax", "kF32ResidualMax", "kIntCountMax", "kRtOutsideUnit", "x16_dev", "x16_sum")
# dmf_problem_copy_out's arrays: name -> DMF_ARRAY_* (V, D, Rt, Rtp, consts hold doubles, D16 / X16 / W16 u16, Dt8 i8, mask_bits u8)
PROBLEM_ARRAYS = {"V": 0, "D": 1, "Rt": 2, "Rtp": 3, "D16": 4, "X16": 5, "W16": 6, "Dt8": 7, "mask_bits": 8, "consts": 9}
# ... and the byte images of X16 / D16 for the row pass (dmf_problem_has_byte_images; u8, [N16 / 16][SD / 64][1024]): ids of their own
PROBLEM_BYTE_IMAGES = {"X8": 10, "D8": 11}
DMF_MODE_PARTIAL = 0
DMF_MODE_UNSUPERVISED = 1
MAX_K = 64  # dmf::kMaxK: largest n_c + n_u the kernels are built for (DMF_ERR_UNSUPPORTED beyond)
# dmf::kSmallMax*: the envelope of dmf_solve_small (S, n_c + n_u, n_u, N * S)
SMALL_MAX_S, SMALL_MAX_K, SMALL_MAX_NU, SMALL_MAX_ELEMENTS = 64, 16, 4, 1 << 20
# dmf::kMidMax*: the envelope of dmf_solve_mid, and the most workgroups it gives one solve
MID_MAX_S, MID_MAX_K, MID_MAX_NU, MID_MAX_ELEMENTS, MID_MAX_W = 64, 16, 4, 1 << 23, 64
MASK_DRAW_MAX_SEGMENTS = 1024  # DMF_MASK_DRAW_MAX_SEGMENTS: the most segments (workgroups) of a mask draw
SVD_MAX_S, SVD_MAX_NC, SVD_MAX_RANK, SVD_MAX_LDS = 512, 64, 64, 160 * 1024  # dmf::kSvdMax*: what the SVD initialiser's kernels take


def svd_project_lds_bytes(n_samples, rank):
    """dmf::svd_project_lds_bytes: the LDS of k_svd_project (E / sigma columns, an 8-row tile, the partial norms)."""
    return 8 * (n_samples * rank + 8 * ((n_samples + 63) // 64 * 64 + 16) + 512)


KERNEL_ROWPASS, KERNEL_GRAM, KERNEL_ALPHA, KERNEL_COST = 0, 1, 2, 3
KERNEL_FAMILIES = ("rowpass", "gram", "alpha", "cost")

_p = C.c_void_p
_i64 = C.c_int64
_dbl_p = C.POINTER(C.c_double)

# name -> (restype, argtypes); every symbol include/demethify_hip.h declares
SIGNATURES = {
    "dmf_status_string": (C.c_char_p, [C.c_int]),
    "dmf_last_error": (C.c_char_p, []),
    "dmf_abi_version": (C.c_int, []),
    "dmf_context_create": (C.c_int, [C.c_int, _p, C.POINTER(_p)]),
    "dmf_context_destroy": (C.c_int, [_p]),
    "dmf_context_synchronize": (C.c_int, [_p]),
    "dmf_context_set_profiling": (C.c_int, [_p, C.c_int]),
    "dmf_context_kernel_time": (C.c_int, [_p, C.c_int, _dbl_p, C.POINTER(_i64)]),
    "dmf_context_reset_kernel_time": (C.c_int, [_p]),
    "dmf_context_set_generic": (C.c_int, [_p, C.c_int]),
    "dmf_context_set_x16": (C.c_int, [_p, C.c_int]),
    "dmf_context_set_rowpass_pair": (C.c_int, [_p, C.c_int]),
    "dmf_context_set_rowpass_defer_c": (C.c_int, [_p, C.c_int]),
    "dmf_context_set_rowpass_bytes": (C.c_int, [_p, C.c_int]),
    "dmf_problem_has_byte_images": (C.c_int, [_p, C.POINTER(C.c_int)]),
    "dmf_rowpass_image_offset": (C.c_int, [C.c_int, C.c_int]),
    "dmf_solver_rowpass_byte_launches": (C.c_int, [_p, C.POINTER(_i64)]),
    "dmf_context_set_stop_confirmation": (C.c_int, [_p, C.c_int]),
    "dmf_problem_create": (C.c_int, [_p, _i64, _i64, _i64, _p, _p, _p, C.c_int, C.POINTER(_p)]),
    "dmf_problem_gather": (C.c_int, [_p, _p, _p, _i64, C.POINTER(_p)]),
    "dmf_problem_gather_device": (C.c_int, [_p, _p, _p, _i64, C.POINTER(_p)]),
    "dmf_problem_mask": (C.c_int, [_p, _p, _p, C.c_int, C.POINTER(_p)]),
    "dmf_solver_holdout_error": (C.c_int, [_p, _p, _dbl_p, C.POINTER(_i64)]),
    "dmf_problem_destroy": (C.c_int, [_p]),
    "dmf_problem_shape": (C.c_int, [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "dmf_problem_gram_known": (C.c_int, [_p, _p, C.c_char_p, _i64]),
    "dmf_problem_report": (C.c_int, [_p, C.POINTER(_i64), _dbl_p]),
    "dmf_problem_copy_out": (C.c_int, [_p, C.c_int, _p, _i64]),
    "dmf_gram_i8_describe": (C.c_int, [_i64, _i64, _i64, _i64, C.c_int, C.c_char_p, _i64]),
    "dmf_solver_gram": (C.c_int, [_p, C.c_int, _p, C.c_char_p, _i64]),
    "dmf_solver_row_moments": (C.c_int, [_p, _p, C.c_char_p, _i64]),
    "dmf_solver_momentum_state": (C.c_int, [_p, _dbl_p, _p, _p]),
    "dmf_cost": (C.c_int, [_p, _p, _p, _i64, _p, C.c_int, _dbl_p]),
    "dmf_cost_describe": (C.c_int, [_i64, _i64, _i64, C.c_int, _i64, C.c_int, C.c_int, C.c_int, C.c_char_p, _i64]),
    "dmf_problem_cost_describe": (C.c_int, [_p, _p, _i64, C.c_char_p, _i64]),
    "dmf_project_simplex": (C.c_int, [_p, _p, _i64, _i64, C.c_double, C.c_int, _p]),
    "dmf_update_u": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i64, C.c_int, C.c_int, _dbl_p, _p, _p]),
    "dmf_update_alpha": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, C.c_int, _dbl_p, _p, _p]),
    "dmf_wls_intercept": (C.c_int, [_p, _p, _p, _i64, C.c_int, C.c_int, _p, C.POINTER(C.c_int)]),
    "dmf_wls_moments": (C.c_int, [_p, _p, _p, _i64, C.c_int, C.c_int, _p]),
    "dmf_nnls_normal": (C.c_int, [_p, _p, _p, _i64, _i64, _p, C.POINTER(C.c_int)]),
    "dmf_svd_gram": (C.c_int, [_p, _p, _p, C.c_int, _p, C.POINTER(_i64)]),
    "dmf_svd_factor": (C.c_int, [_p, _p, _p, _p, _i64, C.c_int, _p, C.POINTER(_p)]),
    "dmf_svd_finish": (C.c_int, [_p, _p, _i64, _i64, _p, _p, C.c_int, _p]),
    "dmf_percentile_axis0": (C.c_int, [_p, _p, _i64, _i64, _p, _i64, C.c_int, _p]),
    "dmf_nanpercentile_axis0": (C.c_int, [_p, _p, _i64, _i64, _p, _i64, C.c_int, _p]),
    "dmf_solver_create": (C.c_int, [_p, _p, _p, _p, _i64, C.c_int, C.c_int, C.POINTER(_p)]),
    "dmf_solver_set_purity": (C.c_int, [_p, _p, C.c_int]),
    "dmf_solver_step": (C.c_int, [_p, _i64, _i64, C.c_double, C.POINTER(_i64), C.POINTER(C.c_int)]),
    "dmf_solver_get": (C.c_int, [_p, C.c_int, _p, _p, _dbl_p, C.POINTER(_i64)]),
    "dmf_solver_match_components": (C.c_int, [_p, _p, _i64, _p, _p]),
    "dmf_solver_get_u_permuted": (C.c_int, [_p, C.POINTER(C.c_int32), _p]),
    "dmf_solver_get_u_by_row": (C.c_int, [_p, _p, _i64, C.POINTER(C.c_int32), _p]),
    "dmf_solver_cost": (C.c_int, [_p, _dbl_p]),
    "dmf_solver_cost_begin": (C.c_int, [_p]),
    "dmf_solver_cost_end": (C.c_int, [_p, _dbl_p]),
    "dmf_solver_destroy": (C.c_int, [_p]),
    "dmf_solver_describe": (C.c_int, [_p, _i64, C.c_char_p, _i64]),
    "dmf_select_describe": (C.c_int, [_i64, _i64, _i64, _i64, C.c_int, C.c_int, _i64, C.c_int, C.c_char_p, _i64]),
    "dmf_u_phase_describe": (C.c_int, [_i64, _i64, _i64, _i64, C.c_int, C.c_int, _i64, C.c_int, C.c_int, C.c_char_p, _i64]),
    "dmf_solver_u_phase_describe": (C.c_int, [_p, _i64, C.c_int, C.c_char_p, _i64]),
    "dmf_solver_stop_info": (C.c_int, [_p, C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(_i64), _dbl_p]),
    "dmf_solver_rowpass_launches": (C.c_int, [_p, C.POINTER(_i64), C.POINTER(_i64)]),
    "dmf_solver_rowpass_schedule_counts": (C.c_int, [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "dmf_table_scan": (C.c_int, [C.c_char_p, C.c_char, C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_int)]),
    "dmf_table_read": (C.c_int, [C.c_char_p, C.c_char, C.c_int, C.c_int, _i64, _p, _i64, C.c_double, _p, _i64, C.c_int]),
    "dmf_host_alloc": (_p, [C.c_size_t, C.POINTER(C.c_int)]),
    "dmf_host_free": (None, [_p, C.c_int]),
    "dmf_write_interval_csv": (C.c_int, [C.c_char_p, C.c_char_p, _p, _p, _i64, C.c_int, C.c_int, C.c_int]),
    "dmf_stage_upload": (C.c_int, [_p, _p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "dmf_stage_free": (C.c_int, [_p, _p]),
    "dmf_stage_download": (C.c_int, [_p, _p, C.c_size_t, _p]),
    "dmf_mask_draw": (C.c_int, [_p, _p, C.POINTER(C.c_int), _i64, _i64, C.c_uint64, C.POINTER(C.c_void_p),
                                C.POINTER(_i64)]),
    "dmf_mask_draw_plan": (C.c_int, [_i64, _i64, C.POINTER(_i64), C.POINTER(_i64)]),
    "dmf_mask_draw_segments": (C.c_int, [_p, _p, C.POINTER(C.c_int), _i64, _i64, C.c_uint64, _i64, C.POINTER(C.c_void_p),
                                         C.POINTER(_i64)]),
    "dmf_mt_jump": (C.c_int, [_p, C.POINTER(C.c_int), C.c_uint64]),
    "dmf_solve": (C.c_int, [_p, _p, _p, _p, _i64, C.c_int, _i64, _i64, C.c_double, C.c_int, _p, _p,
                            _dbl_p, C.POINTER(_i64)]),
    "dmf_solve_small_supported": (C.c_int, [_i64, _i64, _i64, _i64, C.c_int]),
    "dmf_solve_small": (C.c_int, [_p, _p, _i64, _p, _p, _p, _i64, C.c_int, _i64, _i64, C.c_double, _i64, C.c_int, _p, _p, _p, _p]),
    "dmf_solve_small_purity": (C.c_int, [_p, _p, _i64, _p, _p, _p, _p, _i64, C.c_int, _i64, _i64, C.c_double, _i64, C.c_int, _p, _p,
                                         _p, _p]),
    "dmf_solve_small_masked": (C.c_int, [_p, _p, _i64, _p, _p, _p, _i64, C.c_int, _i64, _i64, C.c_double, _i64, C.c_int, _p, _p, _p,
                                         _p, _p, _p]),
    "dmf_solve_mid_supported": (C.c_int, [_i64, _i64, _i64, _i64, C.c_int]),
    "dmf_solve_mid_plan": (C.c_int, [_i64, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "dmf_solve_mid": (C.c_int, [_p, _p, _i64, _p, _p, _p, _i64, C.c_int, _i64, _i64, C.c_double, _i64, _i64, C.c_int, _p, _p, _p,
                                _p]),
    "dmf_solve_mid_purity": (C.c_int, [_p, _p, _i64, _p, _p, _p, _p, _i64, C.c_int, _i64, _i64, C.c_double, _i64, _i64, C.c_int, _p,
                                       _p, _p, _p]),
    "dmf_solve_mid_masked": (C.c_int, [_p, _p, _i64, _p, _p, _p, _i64, C.c_int, _i64, _i64, C.c_double, _i64, _i64, C.c_int, _p, _p,
                                       _p, _p, _p, _p]),
}

_lib = None


class DemethifyHipError(RuntimeError):
    """A C-ABI call returned a non-zero dmf_status."""

    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        msg = f"{where}: status {status}"
        if detail:
            msg += f" ({detail})"
        super().__init__(msg)


def _preload_torch_hip_runtime():
    import importlib.util
    import os

    if os.environ.get("DEMETHIFY_SYSTEM_HIP") == "1":  # (opt out: use the runtime this library was linked against)
        return
    try:
        spec = importlib.util.find_spec("torch")  # (does not import torch)
        if spec is None or not spec.submodule_search_locations:
            return
        cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
        if cand.exists():
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
    except Exception:  # pragma: no cover - no torch, or a wheel without the bundled runtime: nothing to align
        pass


def load():
    """Load the shared library (once) and type every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m demethify_amd._build` "
            "(there is no CPU fallback)")
    # If PyTorch-ROCm lives in this process (bench.py, the multi-GPU drivers), let it bring up its HIP
    # runtime first: torch's wheel bundles its own libamdhip64, and initialising ours before it leaves torch
    # without a device ("no ROCm-capable device is detected").
    import sys

    torch = sys.modules.get("torch")
    if torch is not None:
        try:
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:  # pragma: no cover - torch without a usable GPU: our own checks will report it
            pass
    else:
        # torch is installed but not imported yet (the CLI): a later `import torch` -- the bootstrap's replicate stack,
        # torch.distributed -- would bring a SECOND HIP runtime into the process and find no GPU with it (measured: two
        # libamdhip64 in /proc/self/maps, torch.cuda.is_available() False).  Loading torch's copy of the runtime first
        # makes it the one this library binds to as well -- the configuration bench.py and the test-suite run in --
        # without paying for `import torch` (1.5 s) in runs that never need it.
        _preload_torch_hip_runtime()
    lib = C.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(status: int, where: str):
    if status != DMF_OK:
        lib = load()
        text = lib.dmf_status_string(status).decode()
        err = lib.dmf_last_error().decode()
        raise DemethifyHipError(status, where, f"{text}; {err}" if err else text)
