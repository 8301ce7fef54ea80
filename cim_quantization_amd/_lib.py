"""ctypes binding of libcimq.so (the C ABI declared in include/cimq.h).

The shared library is built in-tree (``python -m cim_quantization_amd.build`` or
``__graft_entry__.build()``) and loaded from this package directory.  There is no
fallback: if the library is missing or was built for another ABI, every compute entry
point raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CIMQ_LIB_PATH") or os.path.join(_HERE, "libcimq.so")
ABI_VERSION = 16
ABI_MINOR = 1  # CIMQ_ABI_MINOR: activation codes (cimq_act_codes, cimq_module_forward_codes)

CIMQ_EINVAL = 1  # include/cimq.h error codes
CIMQ_EUNSUPPORTED = 2
CIMQ_EHIP = 3
CIMQ_INPUT_XQ = 0
CIMQ_INPUT_RAW_LSQ = 1
# cimq_module_route codes (include/cimq.h CIMQ_ROUTE_*)
ROUTE_NAMES = {0: "general", 1: "v3", 2: "fwd5", 3: "v7", 4: "fused", 5: "c1", 6: "gx5", 7: "gw5", 8: "dense", 9: "r6",
               10: "none", 11: "wide"}
CIMQ_ROUTE_R6 = 9
CIMQ_ROUTE_NONE = 10  # route[1] / route[2] under CIMQ_OPT_INFERENCE (ABI 15)
CIMQ_ROUTE_WIDE = 11  # route[0]: cim_fwd_wide_kernel (cimq_wide_abi() == 1)
CIMQ_LSQ_ACCUMULATE_GRADS = 1
CIMQ_LSQ_SKIP_TAIL = 2
CIMQ_LSQ_DEFER_GW = 4
# cimq_conv_desc.adc_variant (include/cimq.h)
CIMQ_ADC_LIBRARY = 0
CIMQ_ADC_STOCHASTIC = 1
CIMQ_ADC_SHIFT_ROUND = 2
CIMQ_ADC_SHIFT_SIGN = 3
CIMQ_ADC_F_PS_INT8 = 0x100
CIMQ_ADC_F_SHIFT_RANGE = 0x200
CIMQ_OPT_RECOMPUTE = 1  # cimq_conv_desc.options (ABI 14)
CIMQ_OPT_INFERENCE = 4  # forward only: nothing written that a backward would read (ABI 15; bit 2 is refused)
CIMQ_EPI_RELU = 1  # cimq_epilogue.flags (ABI 16)
CIMQ_CODES_NO_FLOAT = 1  # cimq_act_codes.flags (ABI 16, minor 1)
CIMQ_POOL_MAX2 = 2  # cimq_module_forward_pool's pool / cimq_net_ext.pool entries (cimq_pool_abi() == 1)
NET_HEAD_FLATTEN = 1  # cimq_net_ext.head_flags: CIMQ_NET_HEAD_FLATTEN

# every symbol include/cimq.h declares
EXPORTED_SYMBOLS = (
    "cimq_abi_version",
    "cimq_abi_minor",
    "cimq_last_error",
    "cimq_query_sizes",
    "cimq_forward",
    "cimq_backward",
    "cimq_module_forward",
    "cimq_module_backward",
    "cimq_module_backward_tail",
    "cimq_module_backward_params",
    "cimq_module_backward_chain",
    "cimq_pending_flush",
    "cimq_pending_jobs",
    "cimq_module_prepare",
    "cimq_shift_prepare_abi",
    "cimq_module_prepare_shift",
    "cimq_module_shift_supported",
    "cimq_module_route",
    "cimq_w4a4_eval_abi",
    "cimq_module_forward_form",
    "cimq_wide_abi",
    "cimq_module_wide_plan",
    "cimq_module_shift_forward",
    "cimq_module_shift_backward",
    "cimq_module_forward_epilogue",
    "cimq_pool_abi",
    "cimq_module_pool_supported",
    "cimq_module_forward_pool",
    "cimq_module_codes_supported",
    "cimq_module_forward_codes",
    "cimq_net_abi",
    "cimq_net_sizes",
    "cimq_net_forward",
    "cimq_net_sizes_ex",
    "cimq_net_forward_ex",
    "cimq_alpha_init",
    "cimq_shift_forward",
    "cimq_shift_backward",
    "cimq_debug_partial_sums",
    "cimq_debug_state_codes",
    "cimq_debug_recompute_codes",
    "cimq_lsq_quantize_forward",
    "cimq_lsq_quantize_workspace_bytes",
    "cimq_lsq_quantize_backward",
    "cimq_qconv_sizes",
    "cimq_qconv_forward",
    "cimq_qconv_backward_scales",
    "cimq_profile_start",
    "cimq_profile_stop",
    "cimq_profile_read",
    "cimq_flat_sgd",
)

KERNEL_IDS = {"fwd": 1, "bwd_gx": 2, "bwd_gw": 3, "prep_act": 4, "fwd_v7": 5, "gx_v8": 6, "gw_v7": 7, "bwd_fused": 8}
# ids 1-4 time every launch of a role (all kernel variants); 5-7 only the v7-path kernels, one
# rocprof symbol family each (the <NBW, NBA, ...> instantiation the workload uses)
KERNEL_SYMBOLS = {1: "cim_fwd_*", 2: "cim_bwd_gx_*", 3: "cim_bwd_gw_*", 4: "prep_act_kernel",
                  5: "cim_fwd_v3_kernel<*, *, *, *, *, *> + cim_fwd5_kernel", 6: "cim_bwd_gx_v8_kernel<*, *, *, *, *, *> + cim_bwd_gx5_kernel",
                  7: "cim_bwd_gw_v7_kernel<*, *, *> + cim_bwd_gw5_kernel", 8: "cim_bwd_fused_kernel<*, *, *> + cim_bwd_gxw5_kernel<*, *, *> (grad_x and grad_w in one launch)"}


class ConvDesc(ctypes.Structure):
    """Mirror of ``cimq_conv_desc``."""

    _fields_ = [
        ("batch", ctypes.c_int32), ("in_channels", ctypes.c_int32),
        ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32),
        ("out_channels", ctypes.c_int32), ("kernel_h", ctypes.c_int32), ("kernel_w", ctypes.c_int32),
        ("stride_h", ctypes.c_int32), ("stride_w", ctypes.c_int32),
        ("pad_h", ctypes.c_int32), ("pad_w", ctypes.c_int32),
        ("xbar", ctypes.c_int32),
        ("bits_w", ctypes.c_int32), ("bits_a", ctypes.c_int32),
        ("bs_w", ctypes.c_int32), ("bs_a", ctypes.c_int32),
        ("adc_bits", ctypes.c_float),
        ("input_kind", ctypes.c_int32),
        ("lsq_qp", ctypes.c_float),
        ("adc_variant", ctypes.c_int32),
        ("seed_lo", ctypes.c_uint32), ("seed_hi", ctypes.c_uint32),
        ("options", ctypes.c_int32),
    ]


class LsqDesc(ctypes.Structure):
    """Mirror of ``cimq_lsq_desc``."""

    _fields_ = [("qn_w", ctypes.c_float), ("qp_w", ctypes.c_float), ("gscale_a", ctypes.c_float),
                ("gscale_w", ctypes.c_float), ("nbits_alpha", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("wprep", ctypes.c_void_p)]


class Epilogue(ctypes.Structure):
    """Mirror of ``cimq_epilogue`` (ABI 16)."""

    _fields_ = [("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("residual", ctypes.c_void_p),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ActCodes(ctypes.Structure):
    """Mirror of ``cimq_act_codes`` (ABI 16, minor 1)."""

    _fields_ = [("x_codes", ctypes.c_void_p), ("out_codes", ctypes.c_void_p), ("out_alpha_act", ctypes.c_void_p),
                ("out_gscale_a", ctypes.c_float), ("out_qp", ctypes.c_float), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class NetLayer(ctypes.Structure):
    """Mirror of ``cimq_net_layer`` (cimq_net_abi() == 1)."""

    _fields_ = [("desc", ctypes.POINTER(ConvDesc)), ("lsq", ctypes.POINTER(LsqDesc)),
                ("weight", ctypes.c_void_p), ("alpha_act", ctypes.c_void_p), ("alpha_weight", ctypes.c_void_p),
                ("alpha_cim", ctypes.c_void_p), ("beta_cim", ctypes.c_void_p), ("binary_mask", ctypes.c_void_p),
                ("signed_act", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p),
                ("epi_flags", ctypes.c_int32), ("in_slot", ctypes.c_int32), ("in_codes", ctypes.c_int32),
                ("out_slot", ctypes.c_int32), ("out_mode", ctypes.c_int32), ("consumer", ctypes.c_int32),
                ("res_slot", ctypes.c_int32), ("res_c0", ctypes.c_int32), ("res_stride", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("ctx", ctypes.c_void_p)]


class NetHead(ctypes.Structure):
    """Mirror of ``cimq_net_head``."""

    _fields_ = [("in_slot", ctypes.c_int32), ("classes", ctypes.c_int32), ("weight", ctypes.c_void_p),
                ("bias", ctypes.c_void_p), ("pooled", ctypes.c_void_p), ("reserved", ctypes.c_int32 * 2)]


class NetDesc(ctypes.Structure):
    """Mirror of ``cimq_net_desc``."""

    _fields_ = [("n_layers", ctypes.c_int32), ("n_slots", ctypes.c_int32), ("layers", ctypes.POINTER(NetLayer)),
                ("head", ctypes.POINTER(NetHead)), ("B", ctypes.c_int32), ("C", ctypes.c_int32),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


class NetExt(ctypes.Structure):
    """Mirror of ``cimq_net_ext`` (cimq_pool_abi() == 1)."""

    _fields_ = [("pool", ctypes.POINTER(ctypes.c_int32)), ("head_flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


NET_HEAD_MAX_C = 8192  # CIMQ_NET_HEAD_MAX_C


class QConvDesc(ctypes.Structure):
    """Mirror of ``cimq_qconv_desc``."""

    _fields_ = [
        ("batch", ctypes.c_int32), ("in_channels", ctypes.c_int32),
        ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32),
        ("out_channels", ctypes.c_int32), ("kernel_h", ctypes.c_int32), ("kernel_w", ctypes.c_int32),
        ("stride_h", ctypes.c_int32), ("stride_w", ctypes.c_int32),
        ("pad_h", ctypes.c_int32), ("pad_w", ctypes.c_int32),
        ("dilation_h", ctypes.c_int32), ("dilation_w", ctypes.c_int32), ("groups", ctypes.c_int32),
        ("code_min", ctypes.c_int32), ("code_max", ctypes.c_int32),
        ("has_bias", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class Pending(ctypes.Structure):
    """Mirror of ``cimq_pending`` (opaque; zero-initialised by ctypes)."""

    _fields_ = [("opaque", ctypes.c_uint64 * 2048)]


class Sizes(ctypes.Structure):
    """Mirror of ``cimq_sizes``."""

    _fields_ = [("ctx_bytes", ctypes.c_size_t), ("fwd_workspace_bytes", ctypes.c_size_t),
                ("bwd_workspace_bytes", ctypes.c_size_t), ("wprep_bytes", ctypes.c_size_t),
                ("module_ctx_bytes", ctypes.c_size_t)]


class PrepareItem(ctypes.Structure):
    """Mirror of ``cimq_prepare_item``."""

    _fields_ = [("desc", ctypes.POINTER(ConvDesc)), ("lsq", ctypes.POINTER(LsqDesc)),
                ("weight", ctypes.c_void_p), ("alpha_act", ctypes.c_void_p), ("alpha_weight", ctypes.c_void_p),
                ("alpha_cim", ctypes.c_void_p), ("binary_mask", ctypes.c_void_p), ("wprep", ctypes.c_void_p)]


class PrepareShiftItem(ctypes.Structure):
    """Mirror of ``cimq_prepare_shift_item`` (cimq_shift_prepare_abi() == 1)."""

    _fields_ = PrepareItem._fields_ + [("beta_cim", ctypes.c_void_p), ("reserved", ctypes.c_int32 * 2)]


_VP = ctypes.c_void_p
_lock = threading.Lock()
_lib = None


class CimqError(RuntimeError):
    pass


def _bind(lib):
    lib.cimq_abi_version.restype = ctypes.c_int
    lib.cimq_abi_version.argtypes = []
    lib.cimq_abi_minor.restype = ctypes.c_int
    lib.cimq_abi_minor.argtypes = []
    lib.cimq_last_error.restype = ctypes.c_char_p
    lib.cimq_last_error.argtypes = []
    lib.cimq_query_sizes.restype = ctypes.c_int
    lib.cimq_query_sizes.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(Sizes)]
    lib.cimq_forward.restype = ctypes.c_int
    lib.cimq_forward.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 11
    lib.cimq_backward.restype = ctypes.c_int
    lib.cimq_backward.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 14
    lib.cimq_module_forward.restype = ctypes.c_int
    lib.cimq_module_forward.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 11
    lib.cimq_module_backward.restype = ctypes.c_int
    lib.cimq_module_backward.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 16
    lib.cimq_module_backward_tail.restype = ctypes.c_int
    lib.cimq_module_backward_tail.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 9
    lib.cimq_module_backward_params.restype = ctypes.c_int
    lib.cimq_module_backward_params.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 10
    lib.cimq_module_backward_chain.restype = ctypes.c_int
    lib.cimq_module_backward_chain.argtypes = ([ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 15 +
                                               [ctypes.POINTER(Pending), _VP])
    lib.cimq_pending_flush.restype = ctypes.c_int
    lib.cimq_pending_flush.argtypes = [ctypes.POINTER(Pending), _VP]
    lib.cimq_pending_jobs.restype = ctypes.c_int
    lib.cimq_pending_jobs.argtypes = [ctypes.POINTER(Pending)]
    lib.cimq_module_prepare.restype = ctypes.c_int
    lib.cimq_module_prepare.argtypes = [ctypes.c_int, ctypes.POINTER(PrepareItem), _VP]
    lib.cimq_shift_prepare_abi.restype = ctypes.c_int
    lib.cimq_shift_prepare_abi.argtypes = []
    lib.cimq_module_prepare_shift.restype = ctypes.c_int
    lib.cimq_module_prepare_shift.argtypes = [ctypes.c_int, ctypes.POINTER(PrepareShiftItem), _VP]
    lib.cimq_module_shift_supported.restype = ctypes.c_int
    lib.cimq_module_shift_supported.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.cimq_module_route.restype = ctypes.c_int
    lib.cimq_module_route.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_int)]
    # (availability symbols of this library; an older one given by CIMQ_LIB_PATH -- the tools that time this tree
    # against its parent load one -- has neither, and stays loadable without them)
    if hasattr(lib, "cimq_w4a4_eval_abi"):
        lib.cimq_w4a4_eval_abi.restype = ctypes.c_int
        lib.cimq_w4a4_eval_abi.argtypes = []
        lib.cimq_module_forward_form.restype = ctypes.c_int
        lib.cimq_module_forward_form.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_int)]
    if hasattr(lib, "cimq_wide_abi"):
        lib.cimq_wide_abi.restype = ctypes.c_int
        lib.cimq_wide_abi.argtypes = []
        lib.cimq_module_wide_plan.restype = ctypes.c_int
        lib.cimq_module_wide_plan.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_int)]
    lib.cimq_module_shift_forward.restype = ctypes.c_int
    lib.cimq_module_shift_forward.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 12
    lib.cimq_module_shift_backward.restype = ctypes.c_int
    lib.cimq_module_shift_backward.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 18
    lib.cimq_module_forward_epilogue.restype = ctypes.c_int
    lib.cimq_module_forward_epilogue.argtypes = ([ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 8 +
                                                 [ctypes.POINTER(Epilogue)] + [_VP] * 4)
    lib.cimq_module_codes_supported.restype = ctypes.c_int
    lib.cimq_module_codes_supported.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_int)]
    lib.cimq_module_forward_codes.restype = ctypes.c_int
    lib.cimq_module_forward_codes.argtypes = ([ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc),
                                               ctypes.POINTER(ActCodes)] + [_VP] * 8 +
                                              [ctypes.POINTER(Epilogue)] + [_VP] * 4)
    lib.cimq_net_abi.restype = ctypes.c_int
    lib.cimq_net_abi.argtypes = []
    lib.cimq_net_sizes.restype = ctypes.c_int
    lib.cimq_net_sizes.argtypes = [ctypes.POINTER(NetDesc)] + [ctypes.POINTER(ctypes.c_size_t)] * 3
    lib.cimq_net_forward.restype = ctypes.c_int
    lib.cimq_net_forward.argtypes = [ctypes.POINTER(NetDesc), _VP, ctypes.POINTER(_VP), ctypes.POINTER(_VP), _VP, _VP,
                                     _VP]
    if hasattr(lib, "cimq_pool_abi"):
        lib.cimq_pool_abi.restype = ctypes.c_int
        lib.cimq_pool_abi.argtypes = []
        lib.cimq_module_pool_supported.restype = ctypes.c_int
        lib.cimq_module_pool_supported.argtypes = [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_int)]
        lib.cimq_module_forward_pool.restype = ctypes.c_int
        lib.cimq_module_forward_pool.argtypes = ([ctypes.POINTER(ConvDesc), ctypes.POINTER(LsqDesc)] + [_VP] * 8 +
                                                 [ctypes.POINTER(Epilogue), ctypes.c_int] + [_VP] * 4)
        lib.cimq_net_sizes_ex.restype = ctypes.c_int
        lib.cimq_net_sizes_ex.argtypes = ([ctypes.POINTER(NetDesc)] + [ctypes.POINTER(ctypes.c_size_t)] * 3 +
                                          [ctypes.POINTER(NetExt)])
        lib.cimq_net_forward_ex.restype = ctypes.c_int
        lib.cimq_net_forward_ex.argtypes = [ctypes.POINTER(NetDesc), _VP, ctypes.POINTER(_VP), ctypes.POINTER(_VP), _VP,
                                            _VP, _VP, ctypes.POINTER(NetExt)]
    lib.cimq_alpha_init.restype = ctypes.c_int
    lib.cimq_alpha_init.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 10
    lib.cimq_shift_forward.restype = ctypes.c_int
    lib.cimq_shift_forward.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 12
    lib.cimq_shift_backward.restype = ctypes.c_int
    lib.cimq_shift_backward.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 16
    lib.cimq_debug_partial_sums.restype = ctypes.c_int
    lib.cimq_debug_partial_sums.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 12
    lib.cimq_debug_state_codes.restype = ctypes.c_int
    lib.cimq_debug_state_codes.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 4
    lib.cimq_debug_recompute_codes.restype = ctypes.c_int
    lib.cimq_debug_recompute_codes.argtypes = [ctypes.POINTER(ConvDesc)] + [_VP] * 7
    _F, _LL, _I = ctypes.c_float, ctypes.c_longlong, ctypes.c_int
    lib.cimq_lsq_quantize_forward.restype = ctypes.c_int
    lib.cimq_lsq_quantize_forward.argtypes = [_VP, _LL, _VP, _F, _F, _I, _VP, _VP]
    lib.cimq_lsq_quantize_workspace_bytes.restype = ctypes.c_size_t
    lib.cimq_lsq_quantize_workspace_bytes.argtypes = [_LL]
    lib.cimq_lsq_quantize_backward.restype = ctypes.c_int
    lib.cimq_lsq_quantize_backward.argtypes = [_VP, _LL, _VP, _F, _F, _I, _VP, _VP, _VP, _VP, _VP]
    lib.cimq_qconv_sizes.restype = ctypes.c_int
    lib.cimq_qconv_sizes.argtypes = [ctypes.POINTER(QConvDesc), ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.POINTER(ctypes.c_size_t)]
    lib.cimq_qconv_forward.restype = ctypes.c_int
    lib.cimq_qconv_forward.argtypes = [ctypes.POINTER(QConvDesc)] + [_VP] * 9
    lib.cimq_qconv_backward_scales.restype = ctypes.c_int
    lib.cimq_qconv_backward_scales.argtypes = [ctypes.POINTER(QConvDesc)] + [_VP] * 8
    lib.cimq_flat_sgd.restype = ctypes.c_int
    lib.cimq_flat_sgd.argtypes = [ctypes.c_longlong, _VP, _VP, _VP, _VP, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                  ctypes.c_int, _VP]
    lib.cimq_profile_start.restype = ctypes.c_int
    lib.cimq_profile_start.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.cimq_profile_read.restype = ctypes.c_int
    lib.cimq_profile_read.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_double)] * 4 + [ctypes.POINTER(ctypes.c_int)]
    lib.cimq_profile_stop.restype = ctypes.c_int
    lib.cimq_profile_stop.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    return lib


def load(path: str | None = None):
    """Load (once) and return the bound library; raises CimqError if unavailable."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise CimqError(f"libcimq.so not found at {p}; build it with "
                            f"`python -m cim_quantization_amd.build` (hipcc --offload-arch=gfx950)")
        lib = _bind(ctypes.CDLL(p))
        v = lib.cimq_abi_version()
        if v != ABI_VERSION:
            raise CimqError(f"libcimq ABI {v} != expected {ABI_VERSION}; rebuild")
        if path is None:
            _lib = lib
        return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().cimq_last_error().decode(errors="replace")
        raise CimqError(f"{what} failed (status {rc}): {msg}")


def make_desc(B, C, H, W, O, KH, KW, stride, padding, xbar, bits_w, bits_a, bs_w, bs_a, adc_bits,
              input_kind=CIMQ_INPUT_XQ, lsq_qp=0.0, adc_variant=CIMQ_ADC_LIBRARY, seed=0, options=0) -> ConvDesc:
    d = ConvDesc()
    d.batch, d.in_channels, d.in_h, d.in_w = int(B), int(C), int(H), int(W)
    d.out_channels, d.kernel_h, d.kernel_w = int(O), int(KH), int(KW)
    d.stride_h, d.stride_w = int(stride[0]), int(stride[1])
    d.pad_h, d.pad_w = int(padding[0]), int(padding[1])
    d.xbar = int(xbar)
    d.bits_w, d.bits_a, d.bs_w, d.bs_a = int(bits_w), int(bits_a), int(bs_w), int(bs_a)
    d.adc_bits = float(adc_bits)
    d.input_kind = int(input_kind)
    d.lsq_qp = float(lsq_qp)
    d.adc_variant = int(adc_variant)
    d.seed_lo, d.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    d.options = int(options)
    return d


def make_lsq_desc(qn_w, qp_w, gscale_a, gscale_w, nbits_alpha, flags=0, wprep=None) -> LsqDesc:
    q = LsqDesc()
    q.qn_w, q.qp_w = float(qn_w), float(qp_w)
    q.gscale_a, q.gscale_w = float(gscale_a), float(gscale_w)
    q.nbits_alpha = int(nbits_alpha)
    q.flags = int(flags)
    q.wprep = wprep
    return q


def make_epilogue(scale, shift, residual=None, relu=False) -> Epilogue:
    """``scale`` / ``shift`` / ``residual``: device addresses (``tensor.data_ptr()``), residual None for none."""
    e = Epilogue()
    e.scale, e.shift, e.residual = scale, shift, residual
    e.flags = CIMQ_EPI_RELU if relu else 0
    e.reserved = 0
    return e


def make_act_codes(x_codes=None, out_codes=None, out_alpha_act=None, out_gscale_a=0.0, out_qp=0.0,
                   no_float=False) -> ActCodes:
    """``x_codes`` / ``out_codes`` / ``out_alpha_act``: device addresses (``tensor.data_ptr()``) or None."""
    io = ActCodes()
    io.x_codes, io.out_codes, io.out_alpha_act = x_codes, out_codes, out_alpha_act
    io.out_gscale_a, io.out_qp = out_gscale_a, out_qp
    io.flags = CIMQ_CODES_NO_FLOAT if no_float else 0
    io.reserved = 0
    return io


def codes_supported(desc):
    """(in_ok, out_ok) of cimq_module_codes_supported for ``desc``."""
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    check(load().cimq_module_codes_supported(ctypes.byref(desc), ctypes.byref(a), ctypes.byref(b)),
          "cimq_module_codes_supported")
    return bool(a.value), bool(b.value)


def make_qconv_desc(B, C, H, W, O, KH, KW, stride, padding, dilation, groups, code_min, code_max,
                    has_bias) -> QConvDesc:
    d = QConvDesc()
    d.batch, d.in_channels, d.in_h, d.in_w = int(B), int(C), int(H), int(W)
    d.out_channels, d.kernel_h, d.kernel_w = int(O), int(KH), int(KW)
    d.stride_h, d.stride_w = int(stride[0]), int(stride[1])
    d.pad_h, d.pad_w = int(padding[0]), int(padding[1])
    d.dilation_h, d.dilation_w = int(dilation[0]), int(dilation[1])
    d.groups = int(groups)
    d.code_min, d.code_max = int(code_min), int(code_max)
    d.has_bias = 1 if has_bias else 0
    return d


def qconv_sizes(desc: QConvDesc):
    f, b = ctypes.c_size_t(), ctypes.c_size_t()
    check(load().cimq_qconv_sizes(ctypes.byref(desc), ctypes.byref(f), ctypes.byref(b)), "cimq_qconv_sizes")
    return f.value, b.value


def module_route(desc: ConvDesc):
    """(forward, grad_x, grad_w) CIMQ_ROUTE_* codes of the module entry points for ``desc``."""
    r = (ctypes.c_int * 3)()
    check(load().cimq_module_route(ctypes.byref(desc), r), "cimq_module_route")
    return tuple(r)


def module_forward_form(desc: ConvDesc):
    """(state format of the forward family: 0 / 2 / 3 / 4 / 8, 1 where the module forward quantises the activation in
    its own row staging) for ``desc`` -- cimq_module_forward_form (cimq_w4a4_eval_abi() == 1)."""
    f = (ctypes.c_int * 2)()
    check(load().cimq_module_forward_form(ctypes.byref(desc), f), "cimq_module_forward_form")
    return tuple(f)


def module_wide_plan(desc: ConvDesc):
    """(ok, channel chunks, output groups, tiles) of the channel-chunked forward for ``desc`` --
    cimq_module_wide_plan (cimq_wide_abi() == 1)."""
    f = (ctypes.c_int * 4)()
    check(load().cimq_module_wide_plan(ctypes.byref(desc), f), "cimq_module_wide_plan")
    return tuple(f)


def pool_abi() -> int:
    """cimq_pool_abi(): 1 where the pooled store and the cimq_net_*_ex calls exist."""
    return int(load().cimq_pool_abi())


def module_pool_supported(desc: ConvDesc) -> bool:
    """Whether cimq_module_forward_pool takes ``desc`` with CIMQ_POOL_MAX2 -- cimq_module_pool_supported."""
    ok = ctypes.c_int(0)
    check(load().cimq_module_pool_supported(ctypes.byref(desc), ctypes.byref(ok)), "cimq_module_pool_supported")
    return bool(ok.value)


def make_net_ext(pool=None, head_flags=0) -> NetExt:
    """``pool``: None, or one entry (0 / CIMQ_POOL_MAX2) per layer of the plan.  The entries' array is kept alive on
    the returned struct."""
    e = NetExt()
    e._pool = (ctypes.c_int32 * len(pool))(*[int(v) for v in pool]) if pool is not None else None
    e.pool = ctypes.cast(e._pool, ctypes.POINTER(ctypes.c_int32)) if e._pool is not None else None
    e.head_flags = int(head_flags)
    return e


def query_sizes(desc: ConvDesc) -> Sizes:
    s = Sizes()
    check(load().cimq_query_sizes(ctypes.byref(desc), ctypes.byref(s)), "cimq_query_sizes")
    return s


class KernelTimer:
    """Sum of HIP-event-measured durations of every launch of one libcimq kernel."""

    def __init__(self, kernel: str, max_launches: int = 65536):
        self.kid = KERNEL_IDS[kernel]
        self.cap = max_launches
        self.total_ms = 0.0
        self.launches = 0
        self.algo_bytes = 0.0
        self.algo_flops = 0.0

    def __enter__(self):
        check(load().cimq_profile_start(self.kid, self.cap), "cimq_profile_start")
        return self

    def __exit__(self, *exc):
        ms, n = ctypes.c_double(), ctypes.c_int()
        b, f = ctypes.c_double(), ctypes.c_double()
        # per launch (cimq_profile_read, ABI 9): duration, algorithmic bytes, logical flops, MFMA ops
        cap = self.cap
        arr = [(ctypes.c_double * cap)() for _ in range(4)]
        got = ctypes.c_int()
        check(load().cimq_profile_read(cap, *arr, ctypes.byref(got)), "cimq_profile_read")
        k = min(cap, got.value)
        self.per_launch = [tuple(a[i] for a in arr) for i in range(k)]
        check(load().cimq_profile_stop(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(b), ctypes.byref(f)),
              "cimq_profile_stop")
        self.total_ms, self.launches = ms.value, n.value
        self.algo_bytes, self.algo_flops = b.value, f.value
        return False
