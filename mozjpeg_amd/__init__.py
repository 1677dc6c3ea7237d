"""mozjpeg_amd -- ctypes binding of libmozjpeg_hip.so (the MI355X-native JPEG encode hot path).

This package is only a thin binding: the product is the shared library built from
mozjpeg_amd/csrc (HIP kernels for gfx950 + C++ host pipeline + C ABI, see include/mozjpeg_hip.h).
There is deliberately NO CPU fallback anywhere: if the library is missing or no GPU is visible the
calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOZJPEG_AMD_LIB") or os.path.join(_HERE, "libmozjpeg_hip.so")   # (the override: A/B runs of a differently built library, tools/gpu_*.sh)

MAX_COMPS, MAX_SCANS = 4, 64
PROFILE_MAX_COMPRESSION = 0x5D083AAD
PROFILE_FASTEST = 0x2AEA5CB4
COLOR_YCC, COLOR_NONE, COLOR_YCC_IN = 0, 1, 2
CS_GRAYSCALE, CS_RGB, CS_YCBCR = 1, 2, 3      # JpegInfo.jpeg_color_space
CS_CMYK, CS_YCCK = 4, 5                       # four-component files (Adobe-style); CS_CMYK is also their one out_color_space
CS_RGB565 = 16                                # JCS_RGB565: DecodeOpts.out_color_space only
OK, EINVAL, EUNSUPPORTED, EHIP, ENOMEM, ETOOSMALL = 0, -1, -2, -3, -4, -5
TAP_PLANE, TAP_COEF_UQ, TAP_COEF_Q, TAP_COEF_Q0, TAP_HUFF_BITS, TAP_HUFF_VALS, TAP_PROG_SCAN_US, TAP_LL_COUNTS = 1, 2, 3, 4, 5, 6, 7, 8
TAP_FINAL_COUNTS = 9


class MjhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mozjpeg_hip error %d: %s" % (code, msg))
        self.code = code


class Scan(C.Structure):
    _fields_ = [("comps_in_scan", C.c_int), ("component_index", C.c_int * MAX_COMPS),
                ("Ss", C.c_int), ("Se", C.c_int), ("Ah", C.c_int), ("Al", C.c_int)]


class Params(C.Structure):
    """Mirror of mjh_params (include/mozjpeg_hip.h) = the cinfo fields the hot path reads."""
    _fields_ = [("image_width", C.c_int), ("image_height", C.c_int), ("input_components", C.c_int),
                ("num_components", C.c_int), ("h_samp_factor", C.c_int * MAX_COMPS),
                ("v_samp_factor", C.c_int * MAX_COMPS), ("quant_tbl_no", C.c_int * MAX_COMPS),
                ("dc_tbl_no", C.c_int * MAX_COMPS), ("ac_tbl_no", C.c_int * MAX_COMPS),
                ("component_id", C.c_int * MAX_COMPS), ("quantval", (C.c_uint16 * 64) * 4),
                ("compress_profile", C.c_int), ("optimize_coding", C.c_int), ("trellis_quant", C.c_int),
                ("trellis_quant_dc", C.c_int), ("overshoot_deringing", C.c_int),
                ("lambda_log_scale1", C.c_float), ("lambda_log_scale2", C.c_float),
                ("restart_interval", C.c_uint), ("restart_in_rows", C.c_int), ("num_scans", C.c_int),
                ("scan_info", Scan * MAX_SCANS), ("optimize_scans", C.c_int), ("write_JFIF_header", C.c_int),
                ("input_pixel_size", C.c_int), ("rgb_offset", C.c_int * 3), ("data_precision", C.c_int),
                ("trellis_num_loops", C.c_int), ("smoothing_factor", C.c_int), ("color_transform", C.c_int),
                ("dc_scan_opt_mode", C.c_int), ("trellis_delta_dc_weight", C.c_float),
                ("use_scans_in_trellis", C.c_int), ("trellis_freq_split", C.c_int),
                ("trellis_eob_opt", C.c_int), ("trellis_q_opt", C.c_int), ("arith_code", C.c_int),
                ("arith_dc_L", C.c_int * 2), ("arith_dc_U", C.c_int * 2), ("arith_ac_K", C.c_int * 2),
                ("trellis_stats_Ah", C.c_int), ("trellis_stats_Al", C.c_int), ("huff_tables_given", C.c_int),
                ("huff_bits", (C.c_uint8 * 17) * 8), ("huff_vals", (C.c_uint8 * 256) * 8), ("dct_method", C.c_int)]


class JpegScan(C.Structure):
    """mjh_jpeg_scan: one scan of a source file as mjh_jpeg_probe found it"""
    _fields_ = [("comps_in_scan", C.c_int), ("component_index", C.c_int * MAX_COMPS), ("dc_tbl_no", C.c_int * MAX_COMPS),
                ("ac_tbl_no", C.c_int * MAX_COMPS), ("restart_interval", C.c_uint), ("data_offset", C.c_size_t),
                ("data_size", C.c_size_t), ("restart_markers", C.c_uint), ("huff_defined", C.c_int), ("huff_bits", (C.c_uint8 * 17) * 8),
                ("huff_vals", (C.c_uint8 * 256) * 8)]


class JpegScanEx(C.Structure):
    """mjh_jpeg_scan_ex: one scan of a progressive source file (mjh_jpeg_probe_ex): the fields of JpegScan, then its spectral
    selection Ss..Se and successive approximation Ah, Al"""
    _fields_ = JpegScan._fields_ + [("Ss", C.c_int), ("Se", C.c_int), ("Ah", C.c_int), ("Al", C.c_int)]


SRC_PROGRESSIVE = 1         # MJH_SRC_PROGRESSIVE
SRC_LOSSLESS = 2            # MJH_SRC_LOSSLESS
SRC_ARITHMETIC = 4          # MJH_SRC_ARITHMETIC
MAX_SRC_SCANS = 64          # MJH_MAX_SRC_SCANS: the cap on the scans of one progressive file
COPY_MODES = {"none": 0, "comments": 1, "all": 2, "all_except_icc": 3, "icc": 4}      # MJH_COPY_*: jpegtran -copy


class JpegArithCond(C.Structure):
    """struct mjh_jpeg_arith_cond: the arithmetic conditioning of tables 0..3 in force at one SOS (mjh_jpeg_arith_cond)"""
    _fields_ = [("dc_L", C.c_int * 4), ("dc_U", C.c_int * 4), ("ac_K", C.c_int * 4)]


class JpegMarker(C.Structure):
    """mjh_jpeg_marker: one saved COM / APPn segment of a source file (mjh_jpeg_markers)"""
    _fields_ = [("marker", C.c_int), ("data_offset", C.c_size_t), ("data_length", C.c_uint)]


def copy_mode(mode):
    """MJH_COPY_* of a -copy name ("none", "comments", "all", "all_except_icc", "icc") or of the number itself"""
    if isinstance(mode, str):
        if mode not in COPY_MODES:
            raise MjhError(EINVAL, "copy mode %r (one of %s)" % (mode, ", ".join(COPY_MODES)))
        return COPY_MODES[mode]
    return int(mode)


class Transform(C.Structure):
    """mjh_transform: a lossless transform of the re-compression path (jpegtran -rotate / -flip / -transpose / -transverse,
    -trim, -perfect, -crop, -grayscale); make one with transform_spec()"""
    _fields_ = [("transform", C.c_int), ("trim", C.c_int), ("perfect", C.c_int), ("grayscale", C.c_int), ("crop", C.c_int),
                ("crop_width", C.c_uint), ("crop_height", C.c_uint), ("crop_xoffset", C.c_uint), ("crop_yoffset", C.c_uint),
                ("crop_width_set", C.c_int), ("crop_height_set", C.c_int), ("crop_xoffset_set", C.c_int), ("crop_yoffset_set", C.c_int)]


class JpegInfo(C.Structure):
    """mjh_jpeg_info: the marker segments of a source file (no entropy decoding)"""
    _fields_ = [("sof_type", C.c_int), ("data_precision", C.c_int), ("image_width", C.c_int), ("image_height", C.c_int),
                ("num_components", C.c_int), ("component_id", C.c_int * MAX_COMPS), ("h_samp_factor", C.c_int * MAX_COMPS),
                ("v_samp_factor", C.c_int * MAX_COMPS), ("quant_tbl_no", C.c_int * MAX_COMPS), ("quant_defined", C.c_int),
                ("quantval", (C.c_uint16 * 64) * 4), ("jpeg_color_space", C.c_int), ("saw_JFIF_marker", C.c_int),
                ("JFIF_major_version", C.c_int), ("JFIF_minor_version", C.c_int), ("density_unit", C.c_int),
                ("X_density", C.c_int), ("Y_density", C.c_int), ("saw_Adobe_marker", C.c_int), ("Adobe_transform", C.c_int),
                ("num_scans", C.c_int), ("scans", JpegScan * 4), ("lossless_psv", C.c_int), ("lossless_pt", C.c_int)]


class DecodeOpts(C.Structure):
    """mjh_decode_opts: what djpeg's -grayscale / -rgb / -nosmooth / -scale / -dct and the extended pixel layouts choose, TurboJPEG's
    bottom-up rows, and the raw sample planes or the DCT coefficients instead of pixels"""
    _fields_ = [("out_color_space", C.c_int), ("pixel_size", C.c_int), ("rgb_offset", C.c_int * 3), ("fancy_upsampling", C.c_int),
                ("scale_num", C.c_int), ("scale_denom", C.c_int), ("dct_method", C.c_int), ("bottom_up", C.c_int), ("raw_planes", C.c_int),
                ("no_dither", C.c_int), ("raw_coefs", C.c_int), ("all_scales", C.c_int),
                ("crop_x", C.c_int), ("crop_y", C.c_int), ("crop_w", C.c_int), ("crop_h", C.c_int)]


class Result(C.Structure):
    """mjh_result: one finished file inside the pinned result arena"""
    _fields_ = [("offset", C.c_uint64), ("size", C.c_uint64)]


_lib = None


def lib():
    """Load libmozjpeg_hip.so; raises if it has not been built (python -m mozjpeg_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MjhError(EHIP, "%s not built: run `python -m mozjpeg_amd.build` (needs hipcc)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.mjh_last_error.restype = C.c_char_p
        L.mjh_version.restype = C.c_char_p
        L.mjh_params_size.restype = C.c_size_t
        if L.mjh_params_size() != C.sizeof(Params):     # mjh_params grows at its end between versions (include/mozjpeg_hip.h)
            raise MjhError(EINVAL, "%s (%s) has a %d-byte mjh_params, this binding a %d-byte one: rebuild"
                           % (LIB_PATH, L.mjh_version().decode(), L.mjh_params_size(), C.sizeof(Params)))
        L.mjh_device_placement.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        L.mjh_params_defaults.argtypes = [C.POINTER(Params)] + [C.c_int] * 7
        L.mjh_params_set_quality.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_int]
        L.mjh_params_simple_progression.argtypes = [C.POINTER(Params)]
        L.mjh_params_search_progression.argtypes = [C.POINTER(Params)]
        L.mjh_encoder_create.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.mjh_encoder_destroy.argtypes = [C.c_void_p]
        L.mjh_encoder_destroy.restype = None
        L.mjh_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
        L.mjh_encode_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        L.mjh_encode_planes_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.mjh_encode_planes_host.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int]
        L.mjh_encode_coefficients_device.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        L.mjh_encode_coefficients_host.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int]
        L.mjh_encoder_sync.argtypes = [C.c_void_p]
        L.mjh_set_inflight.argtypes = [C.c_void_p, C.c_int]
        L.mjh_encoder_params.argtypes = [C.c_void_p]
        L.mjh_encoder_params.restype = C.POINTER(Params)
        L.mjh_pool_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        L.mjh_pool_destroy.argtypes = [C.c_void_p]
        L.mjh_pool_destroy.restype = None
        L.mjh_pool_device_count.argtypes = [C.c_void_p]
        L.mjh_pool_encode_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int,
                                           C.POINTER(C.POINTER(C.c_void_p)), C.POINTER(C.POINTER(C.c_size_t))]
        L.mjh_pool_last_error.argtypes = [C.c_void_p]
        L.mjh_pool_last_error.restype = C.c_char_p
        L.mjh_collect.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(Result)), C.POINTER(C.c_int)]
        L.mjh_wait_input.argtypes = [C.c_void_p]
        L.mjh_host_staging.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.mjh_stage_commit.argtypes = [C.c_void_p, C.c_size_t]
        L.mjh_encode_gather.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int]
        L.mjh_host_alloc.argtypes = [C.c_size_t]
        L.mjh_host_alloc.restype = C.c_void_p
        L.mjh_host_free.argtypes = [C.c_void_p]
        L.mjh_host_free.restype = None
        L.mjh_host_register.argtypes = [C.c_void_p, C.c_size_t]
        L.mjh_host_unregister.argtypes = [C.c_void_p]
        L.mjh_get_jpeg_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
        L.mjh_get_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mjh_get_output_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_void_p)]
        L.mjh_set_debug_taps.argtypes = [C.c_void_p, C.c_int]
        L.mjh_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.mjh_set_profiling_focus.argtypes = [C.c_void_p, C.c_char_p]
        L.mjh_read_tap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]
        L.mjh_component_geometry.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 4
        L.mjh_get_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_char_p)),
                                           C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int)]
        L.mjh_jpeg_probe.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(JpegInfo)]
        if hasattr(L, "mjh_jpeg_probe_ex"):
            L.mjh_jpeg_probe_ex.argtypes = [C.c_char_p, C.c_size_t, C.c_uint, C.POINTER(JpegInfo), C.POINTER(JpegScanEx), C.c_int, C.POINTER(C.c_int)]
            L.mjh_encoder_set_sources.argtypes = [C.c_void_p, C.c_uint]
            L.mjh_decode_prog_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.mjh_params_from_jpeg.argtypes = [C.POINTER(JpegInfo), C.c_int, C.POINTER(Params)]
        L.mjh_transform_parse_crop.argtypes = [C.POINTER(Transform), C.c_char_p]
        L.mjh_params_from_jpeg_transform.argtypes = [C.POINTER(JpegInfo), C.POINTER(Transform), C.c_int, C.POINTER(Params)]
        L.mjh_encoder_set_transform.argtypes = [C.c_void_p, C.POINTER(Transform)]
        L.mjh_transcode_host.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int]
        if hasattr(L, "mjh_jpeg_markers"):      # (absent from an older library loaded for an A/B run)
            L.mjh_jpeg_markers.argtypes = [C.c_char_p, C.c_size_t, C.c_uint, C.c_int, C.POINTER(JpegMarker), C.c_int, C.POINTER(C.c_int)]
            L.mjh_encoder_set_copy_markers.argtypes = [C.c_void_p, C.c_int]
            L.mjh_encoder_set_icc_profile.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        if hasattr(L, "mjh_jpeg_arith_cond"):
            L.mjh_jpeg_arith_cond.argtypes = [C.c_char_p, C.c_size_t, C.c_uint, C.POINTER(JpegArithCond), C.c_int, C.POINTER(C.c_int)]
            L.mjh_decode_arith_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.mjh_transcode_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]
        L.mjh_transcode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
        if hasattr(L, "mjh_decode_host"):             # (absent from an older MOZJPEG_AMD_LIB variant, as below)
            L.mjh_decode_opts_defaults.argtypes = [C.POINTER(DecodeOpts)]
            L.mjh_decode_opts_defaults.restype = None
            L.mjh_decode_host.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(DecodeOpts)]
            L.mjh_get_pixels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
            L.mjh_get_pixels_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
            L.mjh_decode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
            L.mjh_decode_wait.argtypes = [C.c_void_p]
            L.mjh_decode_region.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
            L.mjh_decode_region_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
            L.mjh_get_plane.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
            L.mjh_get_planes_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.mjh_transcode_batch_size.argtypes = [C.c_void_p]
        if hasattr(L, "mjh_get_coefs"):
            L.mjh_get_coefs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
            L.mjh_get_coefs_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)] + [C.POINTER(C.c_int)] * 3
            L.mjh_get_coefs_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        if hasattr(L, "mjh_get_dc_path"):
            L.mjh_get_dc_path.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        if hasattr(L, "mjh_enc_onepass_stats"):       # (absent from a MOZJPEG_AMD_LIB variant built from an older tree: A/B runs against it)
            L.mjh_enc_onepass_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        if hasattr(L, "mjh_final_ac_fused"):
            L.mjh_final_ac_fused.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if hasattr(L, "mjh_enc_pack_groups"):
            L.mjh_enc_pack_groups.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.mjh_enc_scan_positions.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise MjhError(rc, lib().mjh_last_error().decode())


def make_params(width, height, *, quality=75, baseline=False, revert=False, optimize=False,
                notrellis=False, notrellis_dc=False, noovershoot=False, sample=(2, 2), gray=False,
                grayin=False, quant_table=-1, lambda1=None, lambda2=None, restart=None,
                progressive=False, fastcrush=False, precision=8, trellis_loops=1, smooth=0, rgb=False,
                dc_scan_opt=None, dc_ver_weight=None, use_scans_in_trellis=False, trellis_freq_split=0,
                trellis_eob_opt=False, trellis_q_opt=False, arithmetic=False, arith_cond=None, scans=None, gray_sample=None, yccin=False, dct=None,
                dc_tbl=None, ac_tbl=None, no_optimize=False, lossless=None):
    """Parameters with cjpeg's switch vocabulary (cjpeg.c:371-714).  Without `baseline` or
    `revert` this is cjpeg's default: progressive with scan search (`fastcrush`: fixed 9-scan script).
    lossless=(psv, pt): lossless JPEG (SOF3, cjpeg -lossless psv,Pt / jpeg_enable_lossless) with what jpeg_default_colorspace
    makes of the input -- grayscale stays grayscale, RGB becomes a JCS_RGB file (`gray` has no effect, jcmaster.c:1067-1080);
    precision 8, 12 or 16 (12 / 16: uint16 samples).  With `lossless`, scans=[(components, psv, 0, 0, pt), ...] is a lossless script
    (cjpeg -lossless 1 -scans FILE): every component in exactly one scan, each scan with its own predictor and point transform;
    the (psv, pt) of `lossless` itself then only switches the mode on, as in the reference."""
    p = Params()
    L = lib()
    per_comp = isinstance(sample[0], (tuple, list))      # ((h, v) of Y, (h, v) of Cb, (h, v) of Cr): cjpeg -sample HxV,HxV,HxV
    s0 = sample[0] if per_comp else sample
    _chk(L.mjh_params_defaults(C.byref(p), width, height, 1 if grayin else 3, 1 if gray else 0,
                               PROFILE_FASTEST if revert else PROFILE_MAX_COMPRESSION, s0[0], s0[1]))
    if per_comp and p.num_components == 3:
        for i in range(3):
            p.h_samp_factor[i], p.v_samp_factor[i] = sample[i]
    if gray_sample is not None and p.num_components == 1:   # (h, v) of a gray image's one component: cjpeg sets 2x1 for qualities 80..89 (rdswitch.c:566-570)
        p.h_samp_factor[0], p.v_samp_factor[0] = gray_sample
    _chk(L.mjh_params_set_quality(C.byref(p), quality, 1 if baseline else 0, quant_table))
    for i in range(p.num_components):      # table numbers of the application's own (cinfo->comp_info[i].dc_tbl_no / ac_tbl_no)
        if dc_tbl is not None:
            p.dc_tbl_no[i] = dc_tbl[i]
        if ac_tbl is not None:
            p.ac_tbl_no[i] = ac_tbl[i]
        # slots 2 / 3 are empty until the application defines them (the reference aborts on an empty slot): like oracle/refenc.c,
        # a copy of the standard table of the same parity
        for is_ac, t in ((0, p.dc_tbl_no[i]), (1, p.ac_tbl_no[i])):
            if t > 1 and (dc_tbl is not None or ac_tbl is not None):
                bits, vals, nv = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.c_int()
                _chk(L.mjh_std_huffman_table(is_ac, t & 1, C.byref(bits), C.byref(vals), C.byref(nv)))
                k = 2 * t + is_ac
                for j in range(17):
                    p.huff_bits[k][j] = bits[j]
                for j in range(nv.value):
                    p.huff_vals[k][j] = vals[j]
                p.huff_tables_given |= 1 << k
    if optimize:
        p.optimize_coding = 1
    if no_optimize:
        p.optimize_coding = 0               # by hand, whatever the profile set
    if notrellis:
        p.trellis_quant = 0
    if notrellis_dc:
        p.trellis_quant_dc = 0
    if noovershoot:
        p.overshoot_deringing = 0
    if lambda1 is not None:
        p.lambda_log_scale1 = lambda1
    if lambda2 is not None:
        p.lambda_log_scale2 = lambda2
    p.data_precision = precision
    p.trellis_num_loops = trellis_loops
    p.smoothing_factor = smooth
    if dc_scan_opt is not None:
        p.dc_scan_opt_mode = dc_scan_opt        # read by the script builders below
    if dc_ver_weight is not None:
        p.trellis_delta_dc_weight = dc_ver_weight
    p.use_scans_in_trellis = 1 if use_scans_in_trellis else 0
    p.trellis_freq_split = trellis_freq_split
    p.trellis_eob_opt = 1 if trellis_eob_opt else 0
    p.trellis_q_opt = 1 if trellis_q_opt else 0
    p.arith_code = 1 if arithmetic else 0
    if dct == "fast":              # cjpeg -dct fast: JDCT_IFAST
        p.dct_method = 1
    if arith_cond is not None:     # ((L, U, K) of conditioning table 0, (L, U, K) of table 1): cinfo->arith_dc_L / arith_dc_U / arith_ac_K
        for t, (lo, up, kx) in enumerate(arith_cond):
            p.arith_dc_L[t], p.arith_dc_U[t], p.arith_ac_K[t] = lo, up, kx
    if yccin and not grayin:    # in_color_space = JCS_YCbCr: the pixels are Y, Cb, Cr already (null_convert jccolor.c:479)
        p.color_transform = COLOR_YCC_IN
    if rgb:   # cjpeg -rgb: jpeg_set_colorspace(JCS_RGB) (jcparam.c:611-619): all components 1x1 / table 0, ids 'R' 'G' 'B', no JFIF
        p.color_transform = COLOR_NONE
        p.write_JFIF_header = 0
        for i, cid in enumerate(b"RGB"):
            p.component_id[i] = cid
            p.h_samp_factor[i] = p.v_samp_factor[i] = 1
            p.quant_tbl_no[i] = p.dc_tbl_no[i] = p.ac_tbl_no[i] = 0
    if lossless is not None:    # jpeg_enable_lossless: cinfo->Ss = PSV, Se = 0, Ah = 0, Al = Pt -- as a one-scan script (validate_script)
        p.num_components = 1 if grayin else 3
        p.num_scans, p.optimize_scans = 1, 0
        p.scan_info[0].comps_in_scan = p.num_components
        for j in range(p.num_components):
            p.scan_info[0].component_index[j] = j
        p.scan_info[0].Ss, p.scan_info[0].Se, p.scan_info[0].Ah, p.scan_info[0].Al = lossless[0], 0, 0, lossless[1]
    if lossless is not None and not grayin:   # jpeg_default_colorspace in lossless mode: RGB input -> JCS_RGB (jcparam.c:544-546)
        p.color_transform = COLOR_NONE
        p.write_JFIF_header = 0
        for i, cid in enumerate(b"RGB"):
            p.component_id[i] = cid
            p.h_samp_factor[i] = p.v_samp_factor[i] = 1
            p.quant_tbl_no[i] = p.dc_tbl_no[i] = p.ac_tbl_no[i] = 0
    if restart is not None:
        if isinstance(restart, str) and restart.lower().endswith("b"):
            p.restart_interval = int(restart[:-1])
        else:
            p.restart_in_rows = int(restart)
    if revert:
        if progressive:
            _chk(L.mjh_params_simple_progression(C.byref(p)))
    elif lossless is not None:
        p.optimize_scans = 0         # (cjpeg -lossless without -revert fails in the reference: the caller picks the profile)
    elif not baseline:
        # cjpeg's default in the max-compression profile: progressive, scan search unless -fastcrush
        if fastcrush or progressive:
            _chk(L.mjh_params_simple_progression(C.byref(p)))
        else:
            _chk(L.mjh_params_search_progression(C.byref(p)))
    if scans is not None:      # cjpeg -scans: [(component indices, Ss, Se, Ah, Al), ...] replaces the script, no scan search
        if len(scans) > MAX_SCANS:
            raise ValueError("a script of %d scans (at most %d)" % (len(scans), MAX_SCANS))
        p.optimize_scans = 0
        p.num_scans = len(scans)
        if lossless is None and not (scans[0][1] == 0 and scans[0][2] == 63):
            p.optimize_coding = 1          # a progressive script forces optimal tables (jcmaster.c:1091-1094)
        for i, (comps, ss, se, ah, al) in enumerate(scans):
            p.scan_info[i].comps_in_scan = len(comps)
            for j, c in enumerate(comps):
                p.scan_info[i].component_index[j] = c
            p.scan_info[i].Ss, p.scan_info[i].Se, p.scan_info[i].Ah, p.scan_info[i].Al = ss, se, ah, al
    return p


def _src_accept(progressive_sources, lossless_sources, arithmetic_sources=False):
    return (SRC_PROGRESSIVE if progressive_sources else 0) | (SRC_LOSSLESS if lossless_sources else 0) | (SRC_ARITHMETIC if arithmetic_sources else 0)


def jpeg_info(data, progressive_sources=False, lossless_sources=False, arithmetic_sources=False):
    """The marker segments of a JPEG file (mjh_jpeg_probe): frame, tables, colour space, JFIF / Adobe fields, and per scan its
    components, Huffman tables, restart interval and the byte range of its entropy-coded data.  Raises MjhError (EUNSUPPORTED:
    progressive, arithmetic, lossless, 12-bit, 2 components, a four-component file with an Adobe transform other than 0 or 2;
    EINVAL: malformed).  jpeg_color_space is one of CS_GRAYSCALE, CS_RGB, CS_YCBCR and, for the four-component files that
    decode() reads and nothing writes, CS_CMYK (Adobe transform 0, or no Adobe marker) and CS_YCCK (Adobe transform 2).
    progressive_sources=True (mjh_jpeg_probe_ex with MJH_SRC_PROGRESSIVE): a Huffman-coded progressive file is accepted; its
    JpegInfo has sof_type 2 and num_scans 0, and its scans are the list `prog_scans` of JpegScanEx (empty for a sequential file).
    lossless_sources=True (MJH_SRC_LOSSLESS): a Huffman-coded lossless file of 8, 12 or 16 bits is accepted; its JpegInfo has
    sof_type 3 and num_scans 0, and its scans are the list `lossless_scans` of JpegScanEx, Ss the predictor and Al the point
    transform (empty for any other file).
    arithmetic_sources=True (MJH_SRC_ARITHMETIC): an arithmetic-coded file is accepted -- SOF9 (sof_type 9, its scans in `scans`
    as for a Huffman-coded sequential file) and, together with progressive_sources=True, SOF10 (sof_type 10, its scans in
    `prog_scans`).  dc_tbl_no / ac_tbl_no of such a scan are its conditioning table numbers and huff_defined is 0; `arith_cond`
    lists the conditioning in force at every SOS (jpeg_arith_cond)."""
    info = JpegInfo()
    data = bytes(data)
    accept = _src_accept(progressive_sources, lossless_sources, arithmetic_sources)
    if not accept:
        _chk(lib().mjh_jpeg_probe(data, len(data), C.byref(info)))
        return info
    scans, n = (JpegScanEx * MAX_SRC_SCANS)(), C.c_int()
    _chk(lib().mjh_jpeg_probe_ex(data, len(data), accept, C.byref(info), scans, MAX_SRC_SCANS, C.byref(n)))
    info.prog_scans = [scans[i] for i in range(n.value)] if info.sof_type in (2, 10) else []
    if arithmetic_sources:
        info.arith_cond = jpeg_arith_cond(data, progressive_sources, lossless_sources) if info.sof_type in (9, 10) else []
    info.lossless_scans = [scans[i] for i in range(n.value)] if info.sof_type == 3 else []
    info._prog_keep = scans         # (the list's entries are views of this array)
    return info


def jpeg_arith_cond(data, progressive_sources=False, lossless_sources=False):
    """The arithmetic conditioning in force at every SOS of a file (mjh_jpeg_arith_cond with MJH_SRC_ARITHMETIC), in file order:
    [dict(dc_L=[4], dc_U=[4], ac_K=[4]), ...] for tables 0..3.  A file jpeg_info(arithmetic_sources=True) refuses is refused in
    the same words."""
    data = bytes(data)
    lst, n = (JpegArithCond * MAX_SRC_SCANS)(), C.c_int()
    _chk(lib().mjh_jpeg_arith_cond(data, len(data), _src_accept(progressive_sources, lossless_sources, True), lst, MAX_SRC_SCANS, C.byref(n)))
    return [dict(dc_L=list(c.dc_L), dc_U=list(c.dc_U), ac_K=list(c.ac_K)) for c in lst[:n.value]]


def jpeg_markers(data, copy="all", progressive_sources=False, lossless_sources=False, cap=None, arithmetic_sources=False):
    """The COM / APPn segments of a file that a -copy mode saves (mjh_jpeg_markers = the reference's marker_list), in file order:
    [(marker code, data bytes), ...] -- those between the scans and behind the last one too, and JFIF / Adobe segments, which only
    the writing side leaves out.  A file jpeg_info() refuses is refused in the same words.  cap: room for that many (None: as
    many as there are); more raise MjhError(EINVAL) naming the count."""
    data = bytes(data)
    mode, accept = copy_mode(copy), _src_accept(progressive_sources, lossless_sources, arithmetic_sources)
    n = C.c_int()
    room = 64 if cap is None else int(cap)
    while True:
        lst = (JpegMarker * max(room, 1))()
        rc = lib().mjh_jpeg_markers(data, len(data), accept, mode, lst, room, C.byref(n))
        if rc == EINVAL and cap is None and n.value > room:
            room = n.value
            continue
        _chk(rc)
        return [(m.marker, data[m.data_offset:m.data_offset + m.data_length]) for m in lst[:n.value]]


TRANSFORMS = {"flip_h": 1, "flip_v": 2, "transpose": 3, "transverse": 4, "rot90": 5, "rot180": 6, "rot270": 7}   # JXFORM_CODE


def transform_spec(transform=None, trim=False, perfect=False, crop=None, grayscale=False):
    """The Transform of jpegtran's transform switches, or None when they ask for nothing.  transform: one of TRANSFORMS
    ("rot90" = -rotate 90, "flip_h" = -flip horizontal, ...); crop: the -crop string, "WxH+X+Y" with any subset of the numbers."""
    if isinstance(transform, Transform):
        return transform
    if transform is None and crop is None and not (trim or perfect or grayscale):
        return None
    t = Transform()
    if transform is not None:
        if transform not in TRANSFORMS:
            raise MjhError(EINVAL, "transform %r (one of %s)" % (transform, ", ".join(TRANSFORMS)))
        t.transform = TRANSFORMS[transform]
    if crop is not None:
        _chk(lib().mjh_transform_parse_crop(C.byref(t), str(crop).encode()))
    t.trim, t.perfect, t.grayscale = int(bool(trim)), int(bool(perfect)), int(bool(grayscale))
    return t


def params_from_jpeg(data, *, revert=False, optimize=False, progressive=None, fastcrush=False, restart=0,
                     transform=None, trim=False, perfect=False, crop=None, grayscale=False, progressive_sources=False,
                     lossless_sources=False, arithmetic_sources=False, arithmetic=False):
    """Parameters of a `jpegtran -copy none` run on this file (mjh_params_from_jpeg = jpeg_copy_critical_parameters) plus
    jpegtran's switches in make_params' vocabulary.  `data`: the file's bytes or a JpegInfo.
    transform / trim / perfect / crop / grayscale (transform_spec): the parameters of the DESTINATION of that lossless transform
    (mjh_params_from_jpeg_transform); the Transform rides along as `.transform`, and an Encoder made from these parameters
    applies it in transcode_host.  progressive_sources=True: bytes of a progressive file are accepted (jpeg_info); jpegtran copies
    no scan script, so its parameters are those of a sequential file of the same frame.  lossless_sources=True: bytes of a
    lossless file are accepted; its parameters are the lossless ones of the file (make_params(lossless=(psv, pt)) of its first
    scan, its precision and components), for an Encoder that decodes such files -- jpegtran refuses them.
    arithmetic_sources=True: bytes of an arithmetic-coded file are accepted (jpeg_info).  arithmetic=True: jpegtran -arithmetic,
    the result is arithmetic-coded (arith_code), whatever the source was."""
    info = data if isinstance(data, JpegInfo) else jpeg_info(data, progressive_sources, lossless_sources, arithmetic_sources)
    p = Params()
    L = lib()
    t = transform_spec(transform, trim, perfect, crop, grayscale)
    profile = PROFILE_FASTEST if revert else PROFILE_MAX_COMPRESSION
    if t is None:
        _chk(L.mjh_params_from_jpeg(C.byref(info), profile, C.byref(p)))
    else:
        _chk(L.mjh_params_from_jpeg_transform(C.byref(info), C.byref(t), profile, C.byref(p)))
        p.transform = t
    if optimize:
        p.optimize_coding = 1
    if arithmetic:
        p.arith_code = 1
    if restart:
        if isinstance(restart, str) and restart.lower().endswith("b"):
            p.restart_interval = int(restart[:-1])
        else:
            p.restart_in_rows = int(restart)
    if revert:
        if progressive:
            _chk(L.mjh_params_simple_progression(C.byref(p)))
    elif fastcrush:     # (-progressive alone keeps the profile's scan search: jpeg_simple_progression defers to it while optimize_scans is set, jcparam.c:867-870)
        _chk(L.mjh_params_simple_progression(C.byref(p)))
    return p


def _signature(info):
    """what the files of one mjh_transcode_host batch have in common (everything mjh_params_from_jpeg copies; the colour space
    tells a CMYK file from a YCCK one of the same frame)"""
    nc = info.num_components
    used = sorted(set(info.quant_tbl_no[c] for c in range(nc)))
    return (info.image_width, info.image_height, nc, info.jpeg_color_space, info.sof_type == 3, info.data_precision,
            tuple((info.component_id[c], info.h_samp_factor[c], info.v_samp_factor[c], info.quant_tbl_no[c]) for c in range(nc)),
            tuple(bytes(info.quantval[t]) for t in used))


_recompress_encoders = {}


_LOSSLESS_NO_COEFS = "lossless source file (SOF3): it has no DCT coefficients (jpeg_copy_critical_parameters refuses it as well: JERR_NOTIMPL, jctrans.c:83)"


def recompress(files, *, max_batch=64, device=0, progressive_sources=False, lossless_sources=False, arithmetic_sources=False, copy="none", icc=None,
               **switches):
    """Re-compress JPEG files on the GPU: what `jpegtran -copy none` + the switches (revert, optimize, progressive, fastcrush,
    restart) writes for each of them, in input order.  copy: jpegtran's -copy ("none", "comments", "all", "icc": the COM / APPn
    markers of every source that its result keeps, Encoder.set_copy); icc: the bytes of an ICC profile written into every result
    (jpegtran -icc FILE, Encoder.set_icc_profile), in place of the sources' own under "all".  A source is compared with its result
    as it is returned, markers included.  The files are grouped by what a batch must have in common; one encoder
    per group is kept for later calls.  In the max-compression profile without `revert` / `progressive` a source that is
    smaller than its re-coded file is returned as it came (jpegtran.c:171, :774-777).  A file that cannot be re-coded
    (unsupported type, malformed headers, damaged entropy-coded data) gets the MjhError in its slot; the others are unaffected.
    transform / trim / perfect / crop / grayscale (transform_spec): jpegtran's lossless transforms in the same pass; with any of
    them but `perfect` a source is never returned in place of its result (jpegtran clears prefer_smallest), and a file whose
    geometry refuses the request (not perfect, a crop outside the image) gets that MjhError in its slot.
    progressive_sources=True: progressive files are decoded too (Encoder.set_sources); they share batches with sequential files
    of the same frame.  lossless_sources=True is accepted for symmetry with decode(): a lossless file is refused all the same
    (EUNSUPPORTED in its slot), as jpegtran refuses it.  arithmetic_sources=True: arithmetic-coded files (SOF9; SOF10 together
    with progressive_sources=True) are decoded too -- jpegtran from arithmetic to Huffman coding, or to arithmetic again."""
    files = [bytes(f) for f in files]
    out = [None] * len(files)
    groups = {}
    for i, f in enumerate(files):
        try:
            info = jpeg_info(f, progressive_sources, lossless_sources, arithmetic_sources)
        except MjhError as exc:
            out[i] = exc
            continue
        if info.sof_type == 3:
            out[i] = MjhError(EUNSUPPORTED, _LOSSLESS_NO_COEFS)
            continue
        groups.setdefault(_signature(info), (info, []))[1].append(i)
    prefer_smallest = not (switches.get("revert") or switches.get("progressive"))
    # every transform switch clears it as well (jpegtran.c:227, :293, :396-428), -perfect alone does not
    transforming = switches.get("transform") is not None or switches.get("crop") is not None or bool(switches.get("grayscale") or switches.get("trim"))
    if transforming:
        prefer_smallest = False
    key_sw = tuple(sorted((k, bytes(v) if isinstance(v, Transform) else v) for k, v in switches.items()))
    mode, icc = copy_mode(copy), None if icc is None else bytes(icc)
    for sig, (info, idx) in groups.items():
        key = (sig, key_sw, device, LIB_PATH, mode, icc)
        enc = _recompress_encoders.get(key)
        if enc is not None:
            enc.set_sources(progressive=progressive_sources, arithmetic=arithmetic_sources)
        if enc is None or enc.max_batch < min(max_batch, len(idx)):
            if enc is not None:
                enc.close()
            try:
                enc = _recompress_encoders[key] = Encoder(params_from_jpeg(info, **switches), max_batch=min(max_batch, len(idx)), device=device)
                enc.set_sources(progressive=progressive_sources, arithmetic=arithmetic_sources)
                if mode:
                    enc.set_copy(mode)
                if icc is not None:
                    enc.set_icc_profile(icc)
            except MjhError as exc:         # a transform this group's geometry refuses (perfect, a crop outside the image, ...)
                _recompress_encoders.pop(key, None)
                if not (transforming or switches.get("perfect") or exc.code == EUNSUPPORTED):      # (a frame no encoder exists for)
                    raise
                for i in idx:
                    out[i] = exc
                continue
        for o in range(0, len(idx), enc.max_batch):
            part = idx[o:o + enc.max_batch]
            try:
                res = enc.transcode_host([files[i] for i in part], errors="return")
            except MjhError as exc:         # four components: decoded, not written (the encoder refuses the call as a whole)
                if info.num_components != 4 or exc.code != EUNSUPPORTED:
                    raise
                res = [exc] * len(part)
            bad = [k for k, r in enumerate(res) if isinstance(r, MjhError)]
            if bad and len(bad) < len(part):           # the good files of the batch once more, without the damaged ones
                good = [k for k in range(len(part)) if k not in bad]
                again = enc.transcode_host([files[part[k]] for k in good], errors="return")
                for k, r in zip(good, again):
                    res[k] = r
            for k, i in enumerate(part):
                r = res[k]
                if prefer_smallest and not isinstance(r, MjhError) and len(files[i]) < len(r):
                    r = files[i]
                out[i] = r
    return out


PIXEL_LAYOUTS = {"rgb": (3, (0, 1, 2)), "bgr": (3, (2, 1, 0)), "rgbx": (4, (0, 1, 2)), "bgrx": (4, (2, 1, 0)),
                 "xbgr": (4, (3, 2, 1)), "xrgb": (4, (1, 2, 3))}      # name -> pixel_size, rgb_offset (the extended colour spaces)


SCALED_IDCT_SIZES = (1, 2, 4, 8)      # the k of output = input * k / 8 that decode without all_scales=True
ALL_IDCT_SIZES = tuple(range(1, 17))  # with it: the twelve other sizes of jidctint.c as well


def scale_idct_size(num, denom):
    """the IDCT size k that djpeg -scale num/denom decodes with (jpeg_core_output_dimensions, jdmaster.c:105ff): the smallest k in
    1..16 with num * 8 <= denom * k, else 16.  The output is ceil(W k / 8) x ceil(H k / 8)."""
    k = 1
    while k < 16 and num * 8 > denom * k:
        k += 1
    return k


def _parse_scale(scale, all_scales=False):
    """(num, denom) of a pair or a string "M/N"; None is 1/1.  all_scales: every IDCT size in 1..16, not only 1, 2, 4 and 8"""
    if scale is None:
        return 1, 1
    try:
        if isinstance(scale, str):
            num, denom = scale.split("/")
        else:
            num, denom = scale
        num, denom = int(num), int(denom)
    except (TypeError, ValueError):
        raise MjhError(EINVAL, "scale %r (a pair (num, denom) or a string 'M/N')" % (scale,))
    if num < 1 or denom < 1:
        raise MjhError(EINVAL, "scale %d/%d (both at least 1)" % (num, denom))
    if not (-2 ** 31 <= num < 2 ** 31 and -2 ** 31 <= denom < 2 ** 31):
        raise MjhError(EINVAL, "scale %d/%d (beyond an int)" % (num, denom))
    k = scale_idct_size(num, denom)
    if k not in (ALL_IDCT_SIZES if all_scales else SCALED_IDCT_SIZES):
        raise MjhError(EUNSUPPORTED, "scale %d/%d decodes with the %dx%d inverse DCT; the sizes built are 1x1, 2x2, 4x4 and 8x8" % (num, denom, k, k))
    return num, denom


DCT_METHODS = {None: 0, "int": 0, "islow": 0, "fast": 1, "ifast": 1}     # djpeg -dct int / fast -> mjh_decode_opts.dct_method


def _parse_region(crop):
    """(x, y, w, h) of a tuple (x, y, w, h) or of djpeg's -crop string "WxH+X+Y"; w or h 0: to the right / bottom edge"""
    try:
        if isinstance(crop, str):
            size, x, y = crop.split("+")
            w, h = size.lower().split("x")
        else:
            x, y, w, h = crop
        x, y, w, h = int(x), int(y), int(w), int(h)
    except (TypeError, ValueError):
        raise MjhError(EINVAL, "crop %r (a tuple (x, y, w, h) or a string 'WxH+X+Y')" % (crop,))
    if min(x, y, w, h) < 0 or max(x, y, w, h) >= 2 ** 31:
        raise MjhError(EINVAL, "crop %r (no number may be negative or beyond an int)" % (crop,))
    return x, y, w, h


def decode_opts(color=None, layout=None, pixel_size=0, rgb_offset=None, fancy_upsampling=True, scale=None, dct=None, bottom_up=False,
                raw_planes=False, dither=True, raw_coefs=False, all_scales=False, crop=None):
    """DecodeOpts from djpeg's vocabulary.  color: None (the file's default: gray stays gray, a CMYK or YCCK file gives CMYK,
    everything else RGB), "gray" / "grayscale" (-grayscale), "rgb" (-rgb), "rgb565" (-rgb565: 16-bit pixels, with dither=False
    -dither none), "cmyk" (the one output of four-component files: [H, W, 4], C, M, Y, K; pixel_size 0 or 4, rgb_offset is
    ignored) or a CS_* number; layout: a name out of PIXEL_LAYOUTS, or pixel_size and rgb_offset;
    fancy_upsampling=False: -nosmooth; scale: -scale, a pair (num, denom) or a string "M/N" that resolves to 1/8, 2/8, 4/8 or
    8/8 as djpeg resolves it (scale_idct_size) -- with all_scales=True to any k / 8, k in 1..16 (the other sizes of jidctint.c;
    an opt-in because the refusal of those sizes is part of the tested contract); dct: "int" (the default) or "fast" (-dct fast, TurboJPEG's FASTDCT);
    bottom_up=True: the rows last to first (TurboJPEG's BOTTOMUP); raw_planes=True: no pixels, the sample planes (decode_planes);
    raw_coefs=True: nothing of the above, the quantized DCT coefficients (decode_coefficients);
    crop: a region (x, y, w, h), or djpeg's -crop string "WxH+X+Y", in pixels of the scaled image (mjh_decode_opts.crop_*): x moves
    left to a multiple of the iMCU column width as jpeg_crop_scanline moves it and the width grows by as much, so the arrays
    are [h, w_eff, C] (Encoder.decode_region() tells); w or h 0: to the right / bottom edge; None or four zeros: the whole image."""
    o = DecodeOpts()
    lib().mjh_decode_opts_defaults(C.byref(o))
    if crop is not None:
        o.crop_x, o.crop_y, o.crop_w, o.crop_h = _parse_region(crop)
        if (o.crop_x, o.crop_y, o.crop_w, o.crop_h) != (0, 0, 0, 0):
            if raw_planes or raw_coefs:
                raise MjhError(EUNSUPPORTED, "a region (crop) together with %s: they come for the whole image" % ("raw_planes" if raw_planes else "raw_coefs"))
            if scale is not None and scale_idct_size(*_parse_scale(scale, True)) not in SCALED_IDCT_SIZES:
                _parse_scale(scale, all_scales)         # (without all_scales: the refusal of the scale itself comes first)
                raise MjhError(EUNSUPPORTED, "a region (crop) at a size of all_scales: regions are built for the sizes 1x1, 2x2, 4x4 and 8x8")
    if isinstance(color, str):
        names = {"gray": CS_GRAYSCALE, "grayscale": CS_GRAYSCALE, "rgb": CS_RGB, "rgb565": CS_RGB565, "cmyk": CS_CMYK}
        if color not in names:
            raise MjhError(EINVAL, "color %r (None, 'gray', 'rgb', 'rgb565' or 'cmyk')" % (color,))
        o.out_color_space = names[color]
    elif color is not None:
        o.out_color_space = int(color)
    if layout is not None:
        if layout not in PIXEL_LAYOUTS:
            raise MjhError(EINVAL, "layout %r (one of %s)" % (layout, ", ".join(PIXEL_LAYOUTS)))
        pixel_size, rgb_offset = PIXEL_LAYOUTS[layout]
    o.pixel_size = int(pixel_size)
    if rgb_offset is not None:
        o.rgb_offset[:] = [int(v) for v in rgb_offset]
    elif o.out_color_space == CS_RGB565:
        o.rgb_offset[:] = [0, 0, 0]     # (the defaults name 0, 1, 2; a 16-bit pixel has no byte offsets)
    o.fancy_upsampling = int(bool(fancy_upsampling))
    o.scale_num, o.scale_denom = _parse_scale(scale, all_scales)
    o.all_scales = int(bool(all_scales))
    if isinstance(dct, int) and not isinstance(dct, bool):
        o.dct_method = dct
    elif dct in DCT_METHODS:
        o.dct_method = DCT_METHODS[dct]
    else:
        raise MjhError(EINVAL, "dct %r (None, 'int' or 'fast')" % (dct,))
    o.bottom_up = int(bool(bottom_up))
    o.raw_planes = int(bool(raw_planes))
    o.no_dither = int(not dither)
    o.raw_coefs = int(bool(raw_coefs))
    # the library's own checks (plan_pixels), made here as well so that decode() can refuse its options before it groups files
    if o.dct_method not in (0, 1):
        raise MjhError(EINVAL, "dct_method %d of a decode call (0 = JDCT_ISLOW, 1 = JDCT_IFAST)" % o.dct_method)
    if o.out_color_space not in (0, CS_GRAYSCALE, CS_RGB, CS_RGB565, CS_CMYK):
        raise MjhError(EINVAL, "out_color_space %d (0, CS_GRAYSCALE, CS_RGB, CS_RGB565 or CS_CMYK)" % o.out_color_space)
    if o.out_color_space == CS_CMYK:
        if o.pixel_size not in (0, 4):
            raise MjhError(EINVAL, "pixel_size %d of CMYK output (0 or 4)" % o.pixel_size)
        return o
    if o.out_color_space == CS_RGB565:
        if o.pixel_size not in (0, 2):
            raise MjhError(EINVAL, "pixel_size %d of RGB565 output (0 or 2)" % o.pixel_size)
        if list(o.rgb_offset) != [0, 0, 0]:
            raise MjhError(EINVAL, "rgb_offset %d,%d,%d of RGB565 output (all 0)" % tuple(o.rgb_offset))
        return o
    if o.out_color_space == CS_GRAYSCALE:
        if o.pixel_size not in (0, 1):
            raise MjhError(EINVAL, "pixel_size %d of grayscale output (0 or 1)" % o.pixel_size)
    elif o.pixel_size not in ((0, 3, 4) if o.out_color_space == CS_RGB else (0, 1, 3, 4)):     # (the file's default: 1 is a gray file's)
        raise MjhError(EINVAL, "pixel_size %d of RGB output (0, 3 or 4)" % o.pixel_size)
    off = list(o.rgb_offset)
    if off != [0, 0, 0] and o.pixel_size in (0, 3, 4):
        px = o.pixel_size or 3
        if any(v < 0 or v >= px for v in off) or len(set(off)) != 3:
            raise MjhError(EINVAL, "rgb_offset %d,%d,%d of %d-byte pixels" % (off[0], off[1], off[2], px))
    return o


_decode_encoders = {}


def decode(files, *, max_batch=64, device=0, progressive_sources=False, lossless_sources=False, arithmetic_sources=False, **opts):
    """Decode JPEG files to pixels on the GPU: the bytes `djpeg` (+ -grayscale / -rgb / -nosmooth / -scale / -dct fast, see
    decode_opts) writes for each of them, as numpy arrays [H, W, C] ([H, W] for gray) in input order.  A four-component file
    (Adobe-style CMYK or YCCK) gives [H, W, 4], C, M, Y, K -- what tj3Decompress8 gives for TJPF_CMYK, a CMYK file's samples as
    they are, a YCCK file's converted; any other color= for it, and color="cmyk" for any other file, is EUNSUPPORTED
    ("Unsupported color conversion request") in that file's slot.  With scale=,
    [ceil(H k / 8), ceil(W k / 8), C]; with bottom_up=True, the rows last to first.
    The files are grouped by what a batch must have in common, which the scale is not part of; one encoder per group is kept for
    later calls.  A file that cannot be decoded (unsupported type, malformed headers,
    damaged entropy-coded data) gets the MjhError in its slot; the others are unaffected.
    progressive_sources=True: progressive files are decoded too, except those whose blocks djpeg would smooth (an AC coefficient
    of positions 1..9 never sent or not fully refined): EUNSUPPORTED naming block smoothing.
    lossless_sources=True: lossless files (SOF3, 8 / 12 / 16 bits, predictors 1..7, any point transform) are decoded too, to the
    samples djpeg writes: uint8 arrays for 8-bit files, uint16 for 12 and 16 bits, [H, W] or [H, W, 3] ([H, W, 4] for the
    4-sample layouts, the fourth sample 2^precision - 1).  djpeg converts and scales nothing for these files: color= other than
    the file's own is EUNSUPPORTED in the file's slot, scale / dct / fancy_upsampling are ignored.
    arithmetic_sources=True: arithmetic-coded files are decoded too -- SOF9, and SOF10 together with progressive_sources=True
    (the same block-smoothing refusal as for SOF2)."""
    return _decode_grouped(files, max_batch, device, decode_opts(**opts), progressive_sources, lossless_sources, arithmetic_sources)


def yuv_plane_size(info, comp, k=8):
    """(height, width) of plane `comp` of a file decoded at IDCT size k to planar output: TurboJPEG's tj3YUVPlaneWidth / Height of
    the scaled image (turbojpeg.c) restated with the file's own factors -- the scaled size padded to whole MCUs of the full-size
    samples (hmax x vmax), times the component's share: pad(ceil(W k / 8), hmax) * h / hmax."""
    nc = info.num_components
    maxh = max(info.h_samp_factor[c] for c in range(nc))
    maxv = max(info.v_samp_factor[c] for c in range(nc))
    w, h = -(-info.image_width * k // 8), -(-info.image_height * k // 8)
    pw, ph = -(-w // maxh) * maxh, -(-h // maxv) * maxv
    return ph * info.v_samp_factor[comp] // maxv, pw * info.h_samp_factor[comp] // maxh


def decode_planes(files, scale=None, dct=None, *, max_batch=64, device=0, progressive_sources=False, lossless_sources=False, arithmetic_sources=False,
                  all_scales=False):
    """Decode JPEG files to their sample planes on the GPU, without upsampling or colour conversion (TurboJPEG's
    tj3DecompressToYUVPlanes8): per file a list of uint8 arrays [h, w], one per component, of yuv_plane_size(), or the MjhError.
    Every component is transformed at the scale's own size (mjh_decode_opts.raw_planes), so the planes keep the file's
    subsampling at every scale.  A lossless file has no such planes: with lossless_sources=True, EUNSUPPORTED in its slot."""
    return _decode_grouped(files, max_batch, device, decode_opts(scale=scale, dct=dct, raw_planes=True, all_scales=all_scales), progressive_sources, lossless_sources, arithmetic_sources)


def decode_coefficients(files, *, max_batch=64, device=0, progressive_sources=False, lossless_sources=False, arithmetic_sources=False):
    """Decode JPEG files to their quantized DCT coefficients on the GPU (jpeg_read_coefficients): per file a list of int16 arrays
    [height_in_blocks, width_in_blocks, 64], one per component, block-major and in natural order -- what
    Encoder.encode_coefficients_host takes -- or the MjhError in its slot.  The values are the file's own (no limit of +-1023 is
    applied; the entropy coder refuses what it cannot code).  The quantization tables they belong to: jpeg_info(f).quantval.
    A lossless file has no coefficients: with lossless_sources=True, EUNSUPPORTED in its slot."""
    return _decode_grouped(files, max_batch, device, decode_opts(raw_coefs=True), progressive_sources, lossless_sources, arithmetic_sources)


def _decode_grouped(files, max_batch, device, o, progressive_sources=False, lossless_sources=False, arithmetic_sources=False):
    files = [bytes(f) for f in files]
    out = [None] * len(files)
    groups = {}
    for i, f in enumerate(files):
        try:
            info = jpeg_info(f, progressive_sources, lossless_sources, arithmetic_sources)
        except MjhError as exc:
            out[i] = exc
            continue
        groups.setdefault(_signature(info), (info, []))[1].append(i)
    for sig, (info, idx) in groups.items():
        key = (sig, device, LIB_PATH)
        enc = _decode_encoders.get(key)
        if enc is not None:
            enc.set_sources(progressive=progressive_sources, lossless=lossless_sources, arithmetic=arithmetic_sources and info.sof_type != 3)
        if enc is None or enc.max_batch < min(max_batch, len(idx)):
            if enc is not None:
                enc.close()
            try:
                enc = _decode_encoders[key] = Encoder(params_from_jpeg(info, revert=True), max_batch=min(max_batch, len(idx)), device=device)
                enc.set_sources(progressive=progressive_sources, lossless=lossless_sources, arithmetic=arithmetic_sources and info.sof_type != 3)
            except MjhError as exc:         # a frame no encoder exists for (fractional sampling ratios): this group's files alone
                _decode_encoders.pop(key, None)
                if exc.code != EUNSUPPORTED:
                    raise
                for i in idx:
                    out[i] = exc
                continue
        for a in range(0, len(idx), enc.max_batch):
            part = idx[a:a + enc.max_batch]
            try:
                res = enc.decode_host([files[i] for i in part], errors="return", opts=o)
            except MjhError as exc:         # options djpeg refuses for a lossless file (a colour conversion, planes, coefficients),
                # and a colour conversion the reference has none of (CMYK from or to anything else): this group's files alone
                pixels = not (o.raw_planes or o.raw_coefs)
                four = info.num_components == 4
                no_conversion = pixels and (o.out_color_space not in (0, CS_CMYK) if four else o.out_color_space == CS_CMYK)
                # ... and a region this group's files have none of: a four-component or lossless file, an image it does not fit
                region = (o.crop_x, o.crop_y, o.crop_w, o.crop_h) != (0, 0, 0, 0)
                no_region = region and (exc.code == EUNSUPPORTED and (four or info.sof_type == 3) or
                                        exc.code == EINVAL and "exceeds the scaled image dimensions" in str(exc))
                if not no_region and (exc.code != EUNSUPPORTED or not (info.sof_type == 3 or no_conversion)):
                    raise
                res = [exc] * len(part)
            bad = [k for k, r in enumerate(res) if isinstance(r, MjhError)]
            if bad and len(bad) < len(part):           # the good files of the batch once more, without the damaged ones
                good = [k for k in range(len(part)) if k not in bad]
                again = enc.decode_host([files[part[k]] for k in good], errors="return", opts=o)
                for k, r in zip(good, again):
                    res[k] = r
            for k, i in enumerate(part):
                out[i] = res[k]
    return out


def pinned_empty(shape, dtype=np.uint8):
    """numpy array in pinned host memory (mjh_host_alloc): mjh_encode_host reads it by DMA, without a staging copy.
    The memory is released when the array (and every view of it) is gone."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = lib().mjh_host_alloc(nbytes)
    if not ptr:
        raise MjhError(ENOMEM, lib().mjh_last_error().decode())
    buf = (C.c_uint8 * nbytes).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
    import weakref
    weakref.finalize(buf, lib().mjh_host_free, ptr)
    return arr


def _as_batch(params, a):
    """[n, H, W, C] view of one image or a batch; gray images may come without the channel axis ([H, W] / [n, H, W]), which
    only the encoder's geometry can tell apart from a single [H, W, C] image"""
    h, w, c = params.image_height, params.image_width, (1 if params.input_components == 1 else a.shape[-1])
    if params.input_components == 1:
        if a.shape[-1] != 1 or a.shape[-2:] == (h, w):
            a = a[..., None]                   # no channel axis yet
    if a.ndim == 3:
        a = a[None]
    assert a.ndim == 4 and a.shape[1] == h and a.shape[2] == w, "expected [n, %d, %d, C], got %s" % (h, w, a.shape)
    return a


class Pool:
    """One process driving several GPUs (mjh_pool_*): one encoder + one host thread per device, images dealt
    round-robin (image i -> device i mod N), files returned in image order.  devices=None: every visible device."""

    def __init__(self, params, max_batch_per_device=8, devices=None):
        self._h = C.c_void_p()
        self.params = params
        arr = (C.c_int * len(devices))(*devices) if devices else None
        _chk(lib().mjh_pool_create(C.byref(params), max_batch_per_device, arr, len(devices) if devices else 0, C.byref(self._h)))

    @property
    def device_count(self):
        return lib().mjh_pool_device_count(self._h)

    def encode_host(self, frames):
        """frames: uint8 [n, H, W, C] (or uint16 for 12-bit) C-contiguous.  Returns a list of bytes."""
        frames = _as_batch(self.params, np.ascontiguousarray(frames))
        n = frames.shape[0]
        jp, sz = C.POINTER(C.c_void_p)(), C.POINTER(C.c_size_t)()
        rc = lib().mjh_pool_encode_host(self._h, frames.ctypes.data, frames.strides[1], frames.strides[0], n, C.byref(jp), C.byref(sz))
        if rc != OK:
            raise MjhError(rc, lib().mjh_pool_last_error(self._h).decode() or lib().mjh_last_error().decode())
        return [C.string_at(jp[i], sz[i]) for i in range(n)]

    def close(self):
        if self._h:
            lib().mjh_pool_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Encoder:
    """One parameter set + one GPU + device buffers for up to max_batch images."""

    def __init__(self, params, max_batch=1, device=0):
        self._h = C.c_void_p()
        self.params = params
        self.max_batch = max_batch
        _chk(lib().mjh_encoder_create(C.byref(params), max_batch, device, C.byref(self._h)))
        if getattr(params, "transform", None) is not None:      # params_from_jpeg(..., transform=...)
            self.set_transform(params.transform)

    def set_transform(self, transform=None, **spec):
        """The lossless transform of the following transcode calls (mjh_encoder_set_transform): a Transform, transform_spec()'s
        keywords, or None for none.  The encoder's parameters must be the transform's destination (params_from_jpeg)."""
        t = transform_spec(transform, **spec)
        _chk(lib().mjh_encoder_set_transform(self._h, C.byref(t) if t is not None else None))

    def set_sources(self, progressive=True, lossless=False, arithmetic=False):
        """The kinds of source file the following transcode / decode calls take beyond the sequential ones
        (mjh_encoder_set_sources): progressive=True accepts Huffman-coded progressive files, lossless=True lossless ones (decode
        calls of an encoder made from params_from_jpeg of such a file), arithmetic=True arithmetic-coded ones (SOF9; SOF10 when
        progressive is set as well; EINVAL on an encoder made from a lossless file's parameters, which decodes lossless files
        alone); all False is the state of a new encoder."""
        self._progressive = bool(progressive)
        self._lossless = bool(lossless)
        self._arithmetic = bool(arithmetic)
        _chk(lib().mjh_encoder_set_sources(self._h, _src_accept(progressive, lossless, arithmetic)))

    def set_copy(self, mode):
        """The COM / APPn markers the following transcode calls keep (mjh_encoder_set_copy_markers): jpegtran's -copy name
        ("none", "comments", "all", "all_except_icc", "icc") or the MJH_COPY_* number."""
        _chk(lib().mjh_encoder_set_copy_markers(self._h, copy_mode(mode)))

    def set_icc_profile(self, profile):
        """An ICC profile for every file the encoder produces from now on (mjh_encoder_set_icc_profile: cjpeg -icc, jpegtran -icc);
        None clears it."""
        if profile is None:
            _chk(lib().mjh_encoder_set_icc_profile(self._h, None, 0))
        else:
            profile = bytes(profile)
            _chk(lib().mjh_encoder_set_icc_profile(self._h, profile if profile else b"\0", len(profile)))

    def prog_stats(self):
        """levels of scans in the last call's progressive files (first scans are level 0 and count; 0: no progressive file) and the
        milliseconds their refinement levels took (with profiling) (mjh_decode_prog_stats)"""
        lv, ms = C.c_int(), C.c_float()
        _chk(lib().mjh_decode_prog_stats(self._h, C.byref(lv), C.byref(ms)))
        return dict(levels=lv.value, ms=float(ms.value))

    def arith_stats(self):
        """chains (image, scan, restart segment) of the last call's arithmetic-coded files, the launches they took and, with
        profiling, the milliseconds (mjh_decode_arith_stats)"""
        ch, la, ms = C.c_int(), C.c_int(), C.c_float()
        _chk(lib().mjh_decode_arith_stats(self._h, C.byref(ch), C.byref(la), C.byref(ms)))
        return dict(chains=ch.value, launches=la.value, ms=float(ms.value))

    def close(self):
        if self._h:
            lib().mjh_encoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- encode -------------------------------------------------------------------------------
    def encode_host(self, images):
        """images: uint8 ndarray [n, H, W, C] (or [H, W, C]); returns list of bytes."""
        a = _as_batch(self.params, np.ascontiguousarray(images, dtype=np.uint16 if self.params.data_precision > 8 else np.uint8))
        n = a.shape[0]
        _chk(lib().mjh_encode_host(self._h, a.ctypes.data, a.strides[1], a.strides[0], n))
        return [self.get_jpeg(i) for i in range(n)]

    def submit_host(self, images):
        """Asynchronous mjh_encode_host: queues copy + kernels + hand-over and returns.  Pinned arrays (pinned_empty)
        are read in place and must stay untouched until wait_input()/collect(); others are staged by the library."""
        a = images if images.ndim == 4 else images[None]
        assert a.flags.c_contiguous or (a.strides[3] == a.itemsize and a.strides[2] == a.shape[3] * a.itemsize)
        _chk(lib().mjh_encode_host(self._h, a.ctypes.data, a.strides[1], a.strides[0], a.shape[0]))
        return a.shape[0]

    def wait_input(self):
        _chk(lib().mjh_wait_input(self._h))

    def collect(self, age=0, copy=True):
        """Files of the most recent submit_host batch (age 0) or of the one before it (age 1).  copy=False: memoryviews
        into the encoder's pinned result arena (reused by the second submit_host call after the batch's own)."""
        base, res, cnt = C.c_void_p(), C.POINTER(Result)(), C.c_int()
        _chk(lib().mjh_collect(self._h, age, C.byref(base), C.byref(res), C.byref(cnt)))
        out = []
        for i in range(cnt.value):
            mv = (C.c_uint8 * res[i].size).from_address(base.value + res[i].offset)
            out.append(bytes(mv) if copy else memoryview(mv))
        return out

    def encode_device_ptr(self, ptr, row_pitch, image_stride, n, stream=None):
        _chk(lib().mjh_encode_device(self._h, ptr, row_pitch, image_stride, n, stream))

    def encode_tensor(self, t, stream=None):
        """t: torch CUDA tensor [n, H, W, C] (uint8; int16/uint16 storage for 12- and 16-bit), rows contiguous.  Asynchronous.
        stream: None = the torch stream current on t's device (ordered after whatever produced t); "own" = the encoder's
        private stream (the caller guarantees t is complete, e.g. after a synchronize); or a raw hipStream_t value."""
        import torch
        p = self.params
        px = p.input_pixel_size or p.input_components
        es = 2 if p.data_precision > 8 else 1
        assert t.is_cuda and t.dim() == 4 and t.element_size() == es and t.stride(3) == 1 and t.stride(2) == t.shape[3], "layout"
        assert tuple(t.shape[1:]) == (p.image_height, p.image_width, px), "tensor %s does not match the encoder (%d x %d x %d)" % (
            tuple(t.shape), p.image_height, p.image_width, px)
        assert 1 <= t.shape[0] <= self.max_batch
        if stream is None:
            # the torch stream current on t's device; torch's default stream has handle 0, which the C ABI reads as "the
            # encoder's own stream" -- 1 asks for that stream too, but ordered behind everything queued on the null stream
            # so far, i.e. behind whatever produced `t` there
            stream = torch.cuda.current_stream(t.device).cuda_stream or 1
        elif stream == "own":
            stream = None
        self.encode_device_ptr(t.data_ptr(), t.stride(1) * es, t.stride(0) * es, t.shape[0], stream)

    # component planes in (jpeg_write_raw_data / tj3CompressFromYUVPlanes8): no colour conversion
    @staticmethod
    def _plane_args(ptrs, pitches, strides, widths, heights):
        k = len(ptrs)
        pad = lambda v, z: list(v) + [z] * (4 - k)
        return ((C.c_void_p * 4)(*pad(ptrs, None)), (C.c_size_t * 4)(*pad(pitches, 0)), (C.c_size_t * 4)(*pad(strides, 0)),
                (C.c_int * 4)(*pad(widths, 0)), (C.c_int * 4)(*pad(heights, 0)))

    def encode_planes_host(self, planes):
        """planes: one array per component, [n, h_c, w_c] or [h_c, w_c] (uint8; uint16 for 12-bit).  Returns list of bytes."""
        dt = np.uint16 if self.params.data_precision == 12 else np.uint8
        arrs = [np.ascontiguousarray(a if a.ndim == 3 else a[None], dtype=dt) for a in planes]
        n = arrs[0].shape[0]
        args = self._plane_args([a.ctypes.data for a in arrs], [a.strides[1] for a in arrs], [a.strides[0] for a in arrs],
                                [a.shape[2] for a in arrs], [a.shape[1] for a in arrs])
        _chk(lib().mjh_encode_planes_host(self._h, *args, n))
        return [self.get_jpeg(i) for i in range(n)]

    def encode_planes_tensors(self, planes, stream=None):
        """planes: one CUDA tensor [n, h_c, w_c] per component (contiguous rows).  Asynchronous."""
        for t in planes:
            assert t.is_cuda and t.dim() == 3 and t.stride(2) == 1
        es = planes[0].element_size()
        n = planes[0].shape[0]
        args = self._plane_args([t.data_ptr() for t in planes], [t.stride(1) * es for t in planes],
                                [t.stride(0) * es for t in planes], [t.shape[2] for t in planes], [t.shape[1] for t in planes])
        _chk(lib().mjh_encode_planes_device(self._h, *args, n, stream))

    # quantized coefficients in (jpeg_write_coefficients / jpegtran): entropy-coding passes only
    def encode_coefficients_host(self, coefs):
        """coefs: one int16 array per component, [n, hib, wib(+pad), 64] or [hib, wib(+pad), 64], natural order."""
        arrs = [np.ascontiguousarray(a if a.ndim == 4 else a[None], dtype=np.int16) for a in coefs]
        n, k = arrs[0].shape[0], len(arrs)
        pad = lambda v, z: list(v) + [z] * (4 - k)
        _chk(lib().mjh_encode_coefficients_host(self._h, (C.c_void_p * 4)(*pad([a.ctypes.data for a in arrs], None)),
                                                (C.c_size_t * 4)(*pad([a.shape[2] for a in arrs], 0)),
                                                (C.c_size_t * 4)(*pad([a.strides[0] for a in arrs], 0)), n))
        return [self.get_jpeg(i) for i in range(n)]

    def encode_coefficients_tensors(self, coefs, stream=None):
        """coefs: one int16 CUDA tensor [n, hib, wib(+pad), 64] per component, contiguous.  Asynchronous."""
        for t in coefs:
            assert t.is_cuda and t.is_contiguous() and t.dim() == 4 and t.element_size() == 2
        n, k = coefs[0].shape[0], len(coefs)
        pad = lambda v, z: list(v) + [z] * (4 - k)
        _chk(lib().mjh_encode_coefficients_device(self._h, (C.c_void_p * 4)(*pad([t.data_ptr() for t in coefs], None)),
                                                  (C.c_size_t * 4)(*pad([t.shape[2] for t in coefs], 0)),
                                                  (C.c_size_t * 4)(*pad([t.stride(0) * 2 for t in coefs], 0)), n, stream))

    # existing files in (jpegtran -copy none): Huffman decoding on the device, then the entropy-coding passes
    def submit_transcode(self, files):
        """Asynchronous mjh_transcode_host; results through collect() / get_jpeg()."""
        files = [bytes(f) for f in files]
        n = len(files)
        _chk(lib().mjh_transcode_host(self._h, (C.c_char_p * n)(*files), (C.c_size_t * n)(*[len(f) for f in files]), n))
        return n

    def transcode_status(self, i):
        """(code, text) of file i of the last transcode batch (mjh_transcode_status)"""
        t = C.c_char_p()
        rc = lib().mjh_transcode_status(self._h, i, C.byref(t))
        return rc, (t.value or b"").decode()

    def transcode_stats(self):
        """subsequence bytes, synchronisation rounds, host synchronisations and decoder phase times (ms, with profiling) of the last transcode call;
        after a batch decoded with coefficients=True the times end with "export", the export kernel's"""
        a, b, c, ms = C.c_int(), C.c_int(), C.c_int(), (C.c_float * 4)()
        _chk(lib().mjh_transcode_stats(self._h, C.byref(a), C.byref(b), C.byref(c), ms))
        phases = dict(zip(("sync", "prefix", "store", "dc"), [float(x) for x in ms]))
        x = C.c_float()
        if hasattr(lib(), "mjh_get_coefs_ms") and lib().mjh_get_coefs_ms(self._h, C.byref(x)) == OK:
            phases["export"] = float(x.value)       # the last batch was decoded with coefficients=True: k_export_coefs behind the decoder
        return dict(subseq=a.value, rounds=b.value, host_syncs=c.value, ms=phases)

    def enc_onepass_stats(self):
        """the one-walk Huffman coder (MJH_ENC_ONEPASS): whether it is on, and how often its two slower paths ran since the encoder was made"""
        on, a, b = C.c_int(), C.c_ulonglong(), C.c_ulonglong()
        _chk(lib().mjh_enc_onepass_stats(self._h, C.byref(on), C.byref(a), C.byref(b)))
        return dict(enabled=bool(on.value), long_blocks=a.value, big_groups=b.value)

    def enc_pack_groups(self):
        """groups of 256 blocks per workgroup of the one-walk coder (MJH_ENCP_GROUPS): (the encoder's, its second buffer set's or None)"""
        g, t = C.c_int(), C.c_int()
        _chk(lib().mjh_enc_pack_groups(self._h, C.byref(g), C.byref(t)))
        return g.value, (None if t.value < 0 else t.value)

    def final_ac_fused(self):
        """whether the latest batch counted its final AC statistics inside the AC trellis kernels (MJH_FUSE_FINAL_AC): (the encoder's
        latest batch, its second buffer set's or None)"""
        f, t = C.c_int(), C.c_int()
        _chk(lib().mjh_final_ac_fused(self._h, C.byref(f), C.byref(t)))
        return bool(f.value), (None if t.value < 0 else bool(t.value))

    def final_counts(self, image=0):
        """uint32 [4 slots: DC0, AC0, DC1, AC1][256]: the symbol histograms the image's final tables were made from"""
        out = np.empty((4, 256), np.uint32)
        n = C.c_size_t()
        _chk(lib().mjh_read_tap(self._h, TAP_FINAL_COUNTS, image, 0, out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def dc_path(self):
        """the DC trellis kernels of the latest call: None (no DC trellis), "lane" (one lane per chain, MJH_DC_LANES), "dc3", "dc2" or "speculative"""
        v = C.c_int()
        _chk(lib().mjh_get_dc_path(self._h, C.byref(v)))
        return (None, "lane", "dc3", "dc2", "speculative")[v.value]

    def transcode_host(self, files, errors="raise", **transform):
        """files: JPEG byte strings that agree with the encoder's parameters (params_from_jpeg).  Returns the re-coded files.
        transform=..., trim=..., crop=... (transform_spec): set_transform() first; it stays in force for later calls.
        errors="return": no exception for a batch with damaged files -- their slots hold the MjhError, the slots of the good
        files None (nothing of such a batch is handed out: submit the good ones again)."""
        n = len(files)
        if transform:
            self.set_transform(transform_spec(**transform))
        try:
            self.submit_transcode(files)
            return [self.get_jpeg(i) for i in range(n)]
        except MjhError:
            if errors != "return":
                raise
            res = self._file_errors(n)
            if res is None:
                raise
            return res

    # existing files in, pixels out (djpeg): Huffman decoding, inverse DCT, upsampling and colour conversion on the device
    def submit_decode(self, files, opts=None, coefficients=False, **kw):
        """Asynchronous mjh_decode_host (opts: a DecodeOpts, or decode_opts()' keywords); results through get_pixels() /
        pixels_device() -- with coefficients=True (raw_coefs) through get_coefficients() / coefficients_device()."""
        files = [bytes(f) for f in files]
        n = len(files)
        o = opts if opts is not None else decode_opts(raw_coefs=coefficients, **kw)
        _chk(lib().mjh_decode_host(self._h, (C.c_char_p * n)(*files), (C.c_size_t * n)(*[len(f) for f in files]), n, C.byref(o)))
        return n

    def wait_decode(self):
        """Waits for the last decoded batch and raises the MjhError of its first damaged file (mjh_decode_wait): the call between
        submit_decode() and reading the buffer pixels_device() names."""
        _chk(lib().mjh_decode_wait(self._h))

    def _file_errors(self, n):
        """after a failed transcode / decode call of n files: the per-file MjhError / None list, or None when the call was refused as
        a whole (bad options, an encoder that cannot take it) or every file is fine -- then the call's own error is the answer"""
        if lib().mjh_transcode_batch_size(self._h) != n:
            return None
        res = []
        for i in range(n):
            rc, text = self.transcode_status(i)
            res.append(MjhError(rc, text) if rc != OK else None)
        return None if all(r is None for r in res) else res

    def decode_stats(self):
        """width, height (the scaled ones) and pixel size of the last decoded batch, and the times of its two pixel kernels (ms, with profiling)"""
        w, h, px, ms = C.c_int(), C.c_int(), C.c_int(), (C.c_float * 2)()
        _chk(lib().mjh_decode_stats(self._h, C.byref(w), C.byref(h), C.byref(px), ms))
        return dict(width=w.value, height=h.value, pixel_size=px.value, ms=dict(idct=float(ms[0]), upcolor=float(ms[1])))

    def decode_region(self):
        """(x, y, w, h) of the last decoded batch inside the scaled image (mjh_decode_region): x as jpeg_crop_scanline aligns it, w
        grown by what x moved; without crop=, (0, 0, width, height)"""
        v = [C.c_int() for _ in range(4)]
        _chk(lib().mjh_decode_region(self._h, *[C.byref(a) for a in v]))
        return tuple(a.value for a in v)

    def decode_segments(self):
        """(decoded, total) restart segments of the last decoded batch's files (mjh_decode_region_stats): decoded < total when a
        region left segments of sequential Huffman files with restart markers out"""
        a, b = C.c_longlong(), C.c_longlong()
        _chk(lib().mjh_decode_region_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def get_pixels(self, i, out=None):
        """image i of the last decoded batch: uint8 [H, W, C], [H, W] for gray, uint16 [H, W] for RGB565, and for a lossless file its
        samples, uint8 or (12 / 16 bits) uint16 (mjh_get_pixels); out: an array of that shape with contiguous rows to fill instead of a new one"""
        st = self.decode_stats()
        if self._is_lossless():         # samples of 1 byte (8-bit files) or 2: [H, W] or [H, W, samples per pixel]
            dt = np.uint16 if self.params.data_precision > 8 else np.uint8
            spp = st["pixel_size"] // np.dtype(dt).itemsize
            shape = (st["height"], st["width"]) + ((spp,) if spp > 1 else ())
            a = np.empty(shape, dt) if out is None else out
            assert a.shape == shape and a.dtype == dt and a.strides[1:] == np.empty(shape[1:], dt).strides, "expected %s %s" % (np.dtype(dt).name, shape)
            _chk(lib().mjh_get_pixels(self._h, i, a.ctypes.data, a.strides[0]))
            return a
        if st["pixel_size"] == 2:       # RGB565: one uint16 per pixel
            shape = (st["height"], st["width"])
            a = np.empty(shape, np.uint16) if out is None else out
            assert a.shape == shape and a.dtype == np.uint16 and a.strides[1] == 2, "expected uint16 %s" % (shape,)
            _chk(lib().mjh_get_pixels(self._h, i, a.ctypes.data, a.strides[0]))
            return a
        shape = (st["height"], st["width"]) + ((st["pixel_size"],) if st["pixel_size"] > 1 else ())
        a = np.empty(shape, np.uint8) if out is None else out
        assert a.shape == shape and a.dtype == np.uint8 and a.strides[1:] == np.empty(shape[1:], np.uint8).strides, "expected uint8 %s" % (shape,)
        _chk(lib().mjh_get_pixels(self._h, i, a.ctypes.data, a.strides[0]))
        return a

    def _is_lossless(self):
        """the encoder was made from lossless parameters (make_params(lossless=...), params_from_jpeg of a lossless file)"""
        p = self.params
        return 0 < p.num_scans <= MAX_SCANS and p.scan_info[0].Ss != 0 and p.scan_info[0].Se == 0

    def pixels_device(self):
        """(device pointer, row pitch, image stride, decode_stats()) of the last decoded batch (mjh_get_pixels_device); wait_decode() first"""
        base, pitch, stride = C.c_void_p(), C.c_size_t(), C.c_size_t()
        _chk(lib().mjh_get_pixels_device(self._h, C.byref(base), C.byref(pitch), C.byref(stride)))
        return base.value, pitch.value, stride.value, self.decode_stats()

    def get_planes(self, i, info, k):
        """the sample planes of image i of the last batch, decoded with raw_planes at IDCT size k: a list of uint8 [h, w] arrays of
        yuv_plane_size(info, c, k) (mjh_get_plane); info: the JpegInfo of the file"""
        out = []
        for c in range(info.num_components):
            a = np.empty(yuv_plane_size(info, c, k), np.uint8)
            _chk(lib().mjh_get_plane(self._h, i, c, a.ctypes.data, a.strides[0], a.shape[1], a.shape[0]))
            out.append(a)
        return out

    def planes_device(self, comp):
        """(device pointer, row pitch, image stride, width, height) of component comp's plane of the last raw_planes batch
        (mjh_get_planes_device); wait_decode() first"""
        base, pitch, stride, w, h = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
        _chk(lib().mjh_get_planes_device(self._h, comp, C.byref(base), C.byref(pitch), C.byref(stride), C.byref(w), C.byref(h)))
        return base.value, pitch.value, stride.value, w.value, h.value

    def get_coefficients(self, i):
        """the coefficients of image i of the last batch decoded with coefficients=True: one int16 array [height_in_blocks,
        width_in_blocks, 64] per component (mjh_get_coefs)"""
        out = []
        for c in range(self.params.num_components):
            wib, hib = self.geometry(c)[:2]
            a = np.empty((hib, wib, 64), np.int16)
            _chk(lib().mjh_get_coefs(self._h, i, c, a.ctypes.data, wib))
            out.append(a)
        return out

    def coefficients_device(self, comp):
        """(device pointer, image stride in bytes, blocks per row, height in blocks, width in blocks) of component comp's arrays of
        the last batch decoded with coefficients=True (mjh_get_coefs_device): int16 [n, height, blocks per row, 64], contiguous;
        wait_decode() first"""
        base, stride, bpr, hib, wib = C.c_void_p(), C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
        _chk(lib().mjh_get_coefs_device(self._h, comp, C.byref(base), C.byref(stride), C.byref(bpr), C.byref(hib), C.byref(wib)))
        return base.value, stride.value, bpr.value, hib.value, wib.value

    def decode_host(self, files, errors="raise", opts=None, coefficients=False, **kw):
        """files: JPEG byte strings that agree with the encoder's parameters (params_from_jpeg).  Returns their pixels, a list of
        numpy arrays -- or, with raw_planes, per file the list of its sample planes (get_planes), with coefficients=True the list
        of its coefficient arrays (get_coefficients).  errors="return": no exception
        for a batch with damaged files -- their slots hold the MjhError, the slots of the good files None (nothing of such a
        batch is handed out: submit the good ones again)."""
        n = len(files)
        o = opts if opts is not None else decode_opts(raw_coefs=coefficients, **kw)
        try:
            self.submit_decode(files, opts=o)
            if o.raw_coefs:
                return [self.get_coefficients(i) for i in range(n)]
            if o.raw_planes:
                k = 8 if o.scale_num == 0 and o.scale_denom == 0 else scale_idct_size(o.scale_num, o.scale_denom)
                return [self.get_planes(i, jpeg_info(files[i], getattr(self, "_progressive", False), getattr(self, "_lossless", False), getattr(self, "_arithmetic", False)), k) for i in range(n)]
            return [self.get_pixels(i) for i in range(n)]
        except MjhError:
            if errors != "return":
                raise
            res = self._file_errors(n)
            if res is None:
                raise
            return res

    def set_inflight(self, batches):
        """device-resident batches in flight inside the encoder: 2 (default) or 1 (mjh_set_inflight)"""
        _chk(lib().mjh_set_inflight(self._h, batches))

    def sync(self):
        _chk(lib().mjh_encoder_sync(self._h))

    def get_jpeg(self, i):
        n = C.c_size_t()
        _chk(lib().mjh_get_jpeg_size(self._h, i, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        _chk(lib().mjh_get_jpeg(self._h, i, buf.ctypes.data, n.value, C.byref(n)))
        return buf.tobytes()

    def jpeg_size(self, i):
        n = C.c_size_t()
        _chk(lib().mjh_get_jpeg_size(self._h, i, C.byref(n)))
        return n.value

    # -- introspection ------------------------------------------------------------------------
    def set_debug_taps(self, on=True):
        _chk(lib().mjh_set_debug_taps(self._h, int(on)))

    def set_profiling(self, on=True, focus=None):
        """0 off, 1 every kernel, 2 only the interval `focus` (a name out of kernel_times(); None = keep the current choice)"""
        if focus is not None:
            _chk(lib().mjh_set_profiling_focus(self._h, focus.encode()))
        _chk(lib().mjh_set_profiling(self._h, int(on)))

    def geometry(self, c):
        v = [C.c_int() for _ in range(4)]
        _chk(lib().mjh_component_geometry(self._h, c, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)  # wib, hib, pw, ph

    def read_tap(self, what, image=0, comp=0):
        wib, hib, pw, ph = self.geometry(comp if what not in (TAP_HUFF_BITS, TAP_HUFF_VALS, TAP_PROG_SCAN_US) else 0)
        if what == TAP_PROG_SCAN_US:
            out = np.zeros((2, 72), np.uint32)
        elif what == TAP_PLANE:
            out = np.empty((ph, pw), np.uint8)
        elif what == TAP_HUFF_BITS:
            out = np.empty((4, 17), np.uint8)
        elif what == TAP_HUFF_VALS:
            out = np.empty((4, 256), np.uint8)
        else:
            out = np.empty((64, wib * hib), np.int16)
        n = C.c_size_t()
        _chk(lib().mjh_read_tap(self._h, what, image, comp, out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def kernel_times(self):
        names = C.POINTER(C.c_char_p)()
        ms = C.POINTER(C.c_float)()
        cnt = C.c_int()
        _chk(lib().mjh_get_kernel_times(self._h, C.byref(names), C.byref(ms), C.byref(cnt)))
        return [(names[i].decode(), float(ms[i])) for i in range(cnt.value)]
