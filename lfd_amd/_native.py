"""ctypes binding of liblfdmi.so (include/lfdmi.h): the only way Python reaches the GPU path.

There is deliberately no CPU fallback: if the shared library is missing or no HIP device is
usable, every entry point raises.  numpy arrays are passed as host pointers (the library
stages them); objects exposing ``data_ptr()`` (torch CUDA tensors) are passed as device
pointers and used in place.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LFDMI_LIB") or os.path.join(_HERE, "csrc", "liblfdmi.so")   # ($LFDMI_LIB: a developer's variant build)

HOST, DEVICE, HOST_PINNED = 0, 1, 2
U8, F32, F64, F32_BE = 0, 1, 2, 3
PREP_NONE, PREP_BRIGHT, PREP_DIM, PREP_BRIGHT_THEN_DIM = 0, 1, 2, 3
STAGE_GRAY, STAGE_EQU, STAGE_CANNY, STAGE_BOX, STAGE_ERODED, STAGE_EQUALIZED = 0, 1, 2, 3, 4, 5
MAX_SCALES = 4
MAX_CALLS_IN_FLIGHT = 2
MAX_SET_LINES = 64
MAX_MORPH_K = 31

ERR_ARG, ERR_DTYPE, ERR_HIP, ERR_UNSUPPORTED, ERR_CAPACITY, ERR_NOLINES = -1, -2, -3, -4, -5, -6


# every symbol include/lfdmi.h declares (checked by the CPU test-suite)
SYMBOLS = (
    "lfdmi_version", "lfdmi_default_caps", "lfdmi_ctx_create", "lfdmi_ctx_create_sized", "lfdmi_ctx_bytes", "lfdmi_spill_count", "lfdmi_get_stats",
    "lfdmi_ctx_destroy", "lfdmi_last_error", "lfdmi_set_stream", "lfdmi_process_multiscale", "lfdmi_debug_frame_profile", "lfdmi_debug_tail", "lfdmi_debug_trig", "lfdmi_debug_fail_chunk",
    "lfdmi_debug_unit_limits", "lfdmi_debug_unit_split",
    "lfdmi_max_inflight", "lfdmi_prep_u8", "lfdmi_equalize_hist", "lfdmi_dilate", "lfdmi_erode",
    "lfdmi_canny", "lfdmi_gaussian_blur", "lfdmi_fit_min_area_rect", "lfdmi_hough_lines", "lfdmi_hough_accum",
    "lfdmi_hough_dims", "lfdmi_remove_stars", "lfdmi_process_bright", "lfdmi_process_dim",
    "lfdmi_detect_batch", "lfdmi_detect_batch_raw", "lfdmi_host_alloc", "lfdmi_host_free", "lfdmi_fits_read_frames", "lfdmi_fits_read_photoobj", "lfdmi_bz2_find_blocks", "lfdmi_bz2_create", "lfdmi_bz2_destroy", "lfdmi_bz2_last_error", "lfdmi_bz2_decode_batch", "lfdmi_bz2_fetch", "lfdmi_bz2_fetch_many", "lfdmi_bz2_frames", "lfdmi_bz2_reserve", "lfdmi_bz2_timings", "lfdmi_set_stage_images", "lfdmi_get_stage", "lfdmi_get_counters", "lfdmi_enable_timing", "lfdmi_timing_select", "lfdmi_get_timing",
    "lfdmi_timing_slots", "lfdmi_timing_name",
    "lfdmi_detect_batch_begin", "lfdmi_process_multiscale_begin", "lfdmi_end_oldest", "lfdmi_calls_in_flight",
    "lfdmi_default_trail_params", "lfdmi_measure_trails",
    "lfdmi_default_defocus_params", "lfdmi_defocus_bank_create", "lfdmi_defocus_bank_destroy", "lfdmi_defocus_bank_dims",
    "lfdmi_defocus_bank_read", "lfdmi_fit_defocus",
    "lfdmi_default_sky_params", "lfdmi_sky_create", "lfdmi_sky_destroy", "lfdmi_sky_dims", "lfdmi_sky_frames", "lfdmi_sky_normalize",
    "lfdmi_inject_trails",
    "lfdmi_default_mask_params", "lfdmi_mask_trails",
    "lfdmi_default_lc_params", "lfdmi_light_curves",
    "lfdmi_default_strip_params", "lfdmi_trail_strips",
    "lfdmi_default_sub_params", "lfdmi_subtract_trails",
    "lfdmi_default_radon_params", "lfdmi_radon_create", "lfdmi_radon_destroy", "lfdmi_radon_dims", "lfdmi_radon_search",
    "lfdmi_default_radon_lines_params", "lfdmi_radon_search_lines",
    "lfdmi_default_radon_short_params", "lfdmi_radon_search_short",
    "lfdmi_default_radon_wide_params", "lfdmi_radon_search_wide",
    "lfdmi_radon_null", "lfdmi_radon_null_scheme",
    "lfdmi_default_stack_params", "lfdmi_stack_profiles",
    "lfdmi_default_stars_params", "lfdmi_find_stars", "lfdmi_stars_catalog",
    "lfdmi_default_psf_params", "lfdmi_measure_seeing",
    "lfdmi_default_rounds_params", "lfdmi_detect_rounds",
    "lfdmi_default_preview_params", "lfdmi_frame_previews",
    "lfdmi_default_streak_params", "lfdmi_streak_search", "lfdmi_streak_tile",
)


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"liblfdmi error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("lwTresh", C.c_double), ("thetaTresh", C.c_double), ("lineSetTresh", C.c_double),
                ("dro", C.c_double), ("minAreaRectMinLen", C.c_double), ("houghMethod", C.c_double),
                ("nlinesInSet", C.c_int32), ("contoursMode", C.c_int32), ("contoursMethod", C.c_int32),
                ("dilate_kh", C.c_int32), ("dilate_kw", C.c_int32), ("dilateKernel", C.c_void_p),
                ("erode_kh", C.c_int32), ("erode_kw", C.c_int32), ("erodeKernel", C.c_void_p),
                ("minFlux", C.c_double), ("addFlux", C.c_double),
                ("gaussKernel", C.c_int32), ("gaussSigma", C.c_double)]


class UnitLimits(C.Structure):
    """lfdmi_unit_limits: what ``Context.debug_unit_limits`` lowers (0: the compiled default)"""
    _fields_ = [(k, C.c_int64) for k in ("list_pairs", "stage_bytes", "cell_bytes", "render_blocks", "stars_rec_bytes", "stack_part_bytes")]


UNIT_SPLIT_NAMES = ("chunks", "batches", "grid", "launches")


class Caps(C.Structure):
    """lfdmi_caps: per-frame table capacities of a workspace (<= 0: the theoretical maximum)."""
    _fields_ = [("run_cap", C.c_int32), ("key_cap", C.c_int32), ("slot_cap", C.c_int32), ("list_cap", C.c_int32),
                ("peak_cap", C.c_int32), ("min_rho", C.c_double)]


class RsParams(C.Structure):
    _fields_ = [("defaultxy", C.c_int32), ("maxxy", C.c_int32), ("magcount", C.c_int32),
                ("pixscale", C.c_double), ("maxmagdiff", C.c_double), ("filter_cap", C.c_double),
                ("filter_index", C.c_int32)]


class Catalog(C.Structure):
    _fields_ = [("max_obj", C.c_int32), ("count", C.c_void_p), ("rowc", C.c_void_p),
                ("colc", C.c_void_p), ("psfmag", C.c_void_p), ("petro90", C.c_void_p),
                ("nobserve", C.c_void_p), ("ndetect", C.c_void_p), ("loc", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("found", C.c_int32), ("rho", C.c_float), ("theta", C.c_float),
                ("x1", C.c_int32), ("y1", C.c_int32), ("x2", C.c_int32), ("y2", C.c_int32),
                ("n_lines_equ", C.c_int32), ("n_lines_box", C.c_int32), ("detection", C.c_int32),
                ("rejected_by_theta", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RESULT_DTYPE = np.dtype([("status", "<i4"), ("found", "<i4"), ("rho", "<f4"), ("theta", "<f4"),
                         ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"),
                         ("n_lines_equ", "<i4"), ("n_lines_box", "<i4"), ("detection", "<i4"),
                         ("rejected_by_theta", "<i4")])

class TrailParams(C.Structure):
    """lfdmi_trail_params (include/lfdmi.h: trail profiles)."""
    _fields_ = [("half_width", C.c_int32), ("seg_len", C.c_int32), ("n_iter", C.c_int32), ("wing", C.c_int32),
                ("k_sig", C.c_double), ("prof_half", C.c_double), ("prof_step", C.c_double), ("pixscale", C.c_double)]


# lfdmi_trail: one record per frame of lfdmi_measure_trails
TRAIL_DTYPE = np.dtype([("status", "<i4"), ("n_pos", "<i4"), ("n_seg", "<i4"), ("min_valid", "<i4"),
                        ("rho", "<f8"), ("theta", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"),
                        ("background", "<f8"), ("noise", "<f8"), ("peak", "<f8"),
                        ("fwhm", "<f8"), ("fwhm_arcsec", "<f8"), ("depth", "<f8")])
TRAIL_OK, TRAIL_NOT_FOUND, TRAIL_TOO_SHORT, TRAIL_TOO_FAINT = 0, 1, 2, 3


def _make_params(struct, defaults, what, params, convert=None):
    """``struct`` filled by the library's ``defaults`` function, with the given fields replaced (unknown names raise);
    convert: (name, value) -> value, applied to every override."""
    p = struct()
    getattr(lib(), defaults)(C.byref(p))
    names = {k for k, _ in struct._fields_}
    for k, v in params.items():
        if k not in names:
            raise TypeError(f"unknown {what} parameter {k!r}")
        setattr(p, k, convert(k, v) if convert else v)
    return p


def make_trail_params(**params):
    """lfdmi_default_trail_params with the given fields replaced (unknown names raise)."""
    return _make_params(TrailParams, "lfdmi_default_trail_params", "trail", params)


def trail_bins(p):
    """2K+1 profile bins of a TrailParams"""
    return 2 * int(round(p.prof_half / p.prof_step)) + 1


class DefocusParams(C.Structure):
    """lfdmi_defocus_params (include/lfdmi.h: defocus fit)."""
    _fields_ = [("Ro", C.c_double), ("Ri", C.c_double), ("pixscale", C.c_double), ("prof_half", C.c_double),
                ("prof_step", C.c_double), ("wing", C.c_int32), ("ovs", C.c_int32), ("max_shift", C.c_int32),
                ("n_h", C.c_int32), ("n_r", C.c_int32), ("n_seeing", C.c_int32), ("heights", C.POINTER(C.c_double)),
                ("radii", C.POINTER(C.c_double)), ("seeings", C.POINTER(C.c_double)), ("delta_chi2", C.c_double)]


# lfdmi_defocus_model: one record per model of a bank; lfdmi_defocus_fit: one per trail of lfdmi_fit_defocus
DEFOCUS_MODEL_DTYPE = np.dtype([("h_km", "<f8"), ("radius_m", "<f8"), ("sfwhm", "<f8"), ("dfwhm", "<f8"), ("ofwhm", "<f8"),
                                ("depth", "<f8"), ("valid", "<i4"), ("pad", "<i4")])
DEFOCUS_DTYPE = np.dtype([("status", "<i4"), ("shift", "<i4"), ("dof", "<i4"), ("column", "<i4"),
                          ("h_km", "<f8"), ("radius_m", "<f8"), ("seeing_arcsec", "<f8"),
                          ("amplitude", "<f8"), ("offset", "<f8"), ("chi2", "<f8"),
                          ("h_lo", "<f8"), ("h_hi", "<f8"), ("chi2_focus", "<f8"),
                          ("model_ofwhm", "<f8"), ("model_depth", "<f8")])
DEFOCUS_OK, DEFOCUS_NOT_MEASURED, DEFOCUS_GAPS, DEFOCUS_NO_NOISE, DEFOCUS_NO_MODEL = 0, 1, 2, 3, 4


class SkyParamsStruct(C.Structure):
    """lfdmi_sky_params (include/lfdmi.h: sky normalisation)."""
    _fields_ = [("cell", C.c_int32), ("n_clip", C.c_int32), ("filter", C.c_int32), ("mode", C.c_int32),
                ("k_clip", C.c_double), ("target_sigma", C.c_double)]


class SkyFrame(C.Structure):
    """lfdmi_sky_frame: one record per frame of lfdmi_sky_normalize."""
    _fields_ = [("status", C.c_int32), ("ny", C.c_int32), ("nx", C.c_int32), ("n_empty", C.c_int32),
                ("sky", C.c_double), ("sigma", C.c_double), ("gain", C.c_double)]


SKY_DTYPE = np.dtype([("status", "<i4"), ("ny", "<i4"), ("nx", "<i4"), ("n_empty", "<i4"),
                      ("sky", "<f8"), ("sigma", "<f8"), ("gain", "<f8")])
SKY_SUBTRACT, SKY_NORMALISE = 0, 1
SKY_OK, SKY_NO_SKY, SKY_NO_NOISE = 0, 1, 2


def _sky_mode(k, v):
    if k == "mode" and isinstance(v, str):
        return {"subtract": SKY_SUBTRACT, "normalise": SKY_NORMALISE, "normalize": SKY_NORMALISE}[v.lower()]
    return v


def make_sky_params(**params):
    """lfdmi_default_sky_params with the given fields replaced (unknown names raise; mode also as "subtract" / "normalise")."""
    return _make_params(SkyParamsStruct, "lfdmi_default_sky_params", "sky", params, _sky_mode)


# lfdmi_inject_trail: one record per trail of lfdmi_inject_trails (include/lfdmi.h: trail injection)
INJECT_DTYPE = np.dtype([("frame", "<i4"), ("table", "<i4"), ("rho", "<f8"), ("theta", "<f8"), ("t0", "<f8"), ("t1", "<f8"),
                         ("amplitude", "<f8")])
INJECT_MAX_TABLE = 4097


class MaskSegment(C.Structure):
    """lfdmi_mask_segment: one record per segment of lfdmi_mask_trails (include/lfdmi.h: trail masks)."""
    _fields_ = [("frame", C.c_int32), ("bits", C.c_uint8), ("pad", C.c_uint8 * 3),
                ("x1", C.c_double), ("y1", C.c_double), ("x2", C.c_double), ("y2", C.c_double),
                ("half", C.c_double), ("cap", C.c_double), ("fill", C.c_double)]


class MaskParamsStruct(C.Structure):
    """lfdmi_mask_params (include/lfdmi.h: trail masks)."""
    _fields_ = [("fill_mode", C.c_int32), ("clear", C.c_int32)]


MASK_SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("bits", "u1"), ("pad", "u1", (3,)), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"),
                               ("y2", "<f8"), ("half", "<f8"), ("cap", "<f8"), ("fill", "<f8")])
# lfdmi_mask_stat: one record per segment
MASK_STAT_DTYPE = np.dtype([("status", "<i4"), ("n_pix", "<i4")])
MASK_OK, MASK_BAD_SEGMENT, MASK_EMPTY = 0, 1, 2
MASK_FILL_NONE, MASK_FILL_ZERO, MASK_FILL_NAN, MASK_FILL_VALUE = 0, 1, 2, 3
MASK_FILLS = {"none": MASK_FILL_NONE, "zero": MASK_FILL_ZERO, "nan": MASK_FILL_NAN, "value": MASK_FILL_VALUE}


def _mask_fill(k, v):
    if k == "fill_mode" and isinstance(v, str):
        try:
            return MASK_FILLS[v.lower()]
        except KeyError:
            raise ValueError(f"fill must be one of {sorted(MASK_FILLS)}, not {v!r}") from None
    return int(v)


def make_mask_params(**params):
    """lfdmi_default_mask_params with the given fields replaced (unknown names raise; fill_mode also by name)."""
    return _make_params(MaskParamsStruct, "lfdmi_default_mask_params", "mask", params, _mask_fill)


class LcParamsStruct(C.Structure):
    """lfdmi_lc_params (include/lfdmi.h: light curves)."""
    _fields_ = [("sec_len", C.c_double), ("clip", C.c_float), ("min_core", C.c_int32), ("min_sky", C.c_int32)]


LC_PARAMS = LcParamsStruct
# lfdmi_lc_segment: one record per segment of lfdmi_light_curves; lfdmi_lc: its result; lfdmi_lc_section: one per section
LC_SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("pad", "<i4"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"),
                             ("half", "<f8"), ("bg_in", "<f8"), ("bg_out", "<f8")])
LC_DTYPE = np.dtype([("status", "<i4"), ("n_sec", "<i4"), ("n_ok", "<i4"), ("first_ok", "<i4"), ("last_ok", "<i4"),
                     ("peak_section", "<i4"), ("dof", "<i4"), ("pad", "<i4"),
                     ("mean_rate", "<f8"), ("mean_rate_err", "<f8"), ("chi2", "<f8"), ("peak_rate", "<f8"), ("length", "<f8"),
                     ("flux", "<f8"), ("flux_err", "<f8")])
LC_SECTION_DTYPE = np.dtype([("status", "<i4"), ("n_geom", "<i4"), ("n_core", "<i4"), ("n_sky", "<i4"),
                             ("q_core", "<i8"), ("q_sky", "<i8"), ("t0", "<f8"), ("t1", "<f8"),
                             ("mean", "<f8"), ("bkg", "<f8"), ("sb", "<f8"), ("flux", "<f8"), ("flux_err", "<f8"),
                             ("rate", "<f8"), ("rate_err", "<f8"), ("coverage", "<f8")])
LC_OK, LC_BAD_SEGMENT, LC_TOO_LONG, LC_EMPTY = 0, 1, 2, 3
LC_SEC_OK, LC_SEC_LOW, LC_SEC_EMPTY = 0, 1, 2
LC_MAX_SECTIONS = 1024
LC_MAX_BG = 64.0


def make_lc_params(**params):
    """lfdmi_default_lc_params with the given fields replaced (unknown names raise)."""
    return _make_params(LcParamsStruct, "lfdmi_default_lc_params", "light curve", params)


class StripParamsStruct(C.Structure):
    """lfdmi_strip_params (include/lfdmi.h: trail strips)."""
    _fields_ = [("sec_len", C.c_double), ("step", C.c_double), ("wing", C.c_double), ("k_mom", C.c_double), ("clip", C.c_float),
                ("min_core", C.c_int32), ("min_wing", C.c_int32), ("pad", C.c_int32)]


STRIP_PARAMS = StripParamsStruct
# lfdmi_strip_segment: one record per segment of lfdmi_trail_strips; lfdmi_strip: its result; lfdmi_strip_section: one per
# section; lfdmi_strip_cell: one per (section, offset bin)
STRIP_SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("pad", "<i4"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"),
                                ("half", "<f8")])
STRIP_DTYPE = np.dtype([("status", "<i4"), ("n_sec", "<i4"), ("n_off", "<i4"), ("K", "<i4"), ("n_ok", "<i4"), ("n_mom", "<i4"),
                        ("dev_section", "<i4"), ("pad", "<i4"), ("mean_centre", "<f8"), ("mean_width", "<f8"), ("max_dev", "<f8")])
STRIP_SECTION_DTYPE = np.dtype([("status", "<i4"), ("n_geom", "<i4"), ("n_core", "<i4"), ("n_wing", "<i4"), ("t0", "<f8"), ("t1", "<f8"),
                                ("bkg", "<f8"), ("rate", "<f8"), ("rate_err", "<f8"), ("centre", "<f8"), ("width", "<f8")])
STRIP_CELL_DTYPE = np.dtype([("n_geom", "<i4"), ("n", "<i4"), ("q", "<i8")])
STRIP_OK, STRIP_BAD_SEGMENT, STRIP_TOO_LONG, STRIP_EMPTY = 0, 1, 2, 3
STRIP_SEC_OK, STRIP_SEC_LOW, STRIP_SEC_EMPTY = 0, 1, 2
STRIP_MAX_SECTIONS = 1024
STRIP_MAX_OFF = 129


def make_strip_params(**params):
    """lfdmi_default_strip_params with the given fields replaced (unknown names raise)."""
    if "pad" in params:
        raise TypeError("unknown strip parameter 'pad'")
    return _make_params(StripParamsStruct, "lfdmi_default_strip_params", "strip", params)


def strip_cells_needed(segs, p, max_sections):
    """the largest n_sec * n_off of the segments that fit max_sections rows (step 2 of the trail strips, in the header's
    operations), at least 1: the ``max_cells`` with which no such segment is TOO_LONG"""
    most = 1
    inv_s, inv_u = np.float64(1.0) / np.float64(p.sec_len), np.float64(1.0) / np.float64(p.step)
    for s in segs:
        with np.errstate(all="ignore"):
            dx, dy = np.float64(s["x2"]) - np.float64(s["x1"]), np.float64(s["y2"]) - np.float64(s["y1"])
            ns = np.ceil(np.sqrt(dx * dx + dy * dy) * inv_s)
            kk = np.ceil(np.float64(s["half"]) * inv_u - np.float64(0.5))
        if not (np.isfinite(ns) and np.isfinite(kk)) or ns > max_sections or 2 * kk + 1 > STRIP_MAX_OFF:
            continue
        most = max(most, max(1, int(ns)) * (2 * max(0, int(kk)) + 1))
    return most


class SubParamsStruct(C.Structure):
    """lfdmi_sub_params (include/lfdmi.h: trail subtraction)."""
    _fields_ = [("sec_len", C.c_double), ("step", C.c_double), ("wing", C.c_double), ("clip", C.c_float), ("smooth", C.c_int32),
                ("min_sec", C.c_int32), ("min_n", C.c_int32), ("min_wing", C.c_int32), ("apply", C.c_int32)]


SUB_PARAMS = SubParamsStruct
# lfdmi_sub: one record per segment of lfdmi_subtract_trails (its segments are lfdmi_strip_segment records)
SUB_DTYPE = np.dtype([("status", "<i4"), ("n_sec", "<i4"), ("n_off", "<i4"), ("K", "<i4"), ("n_usable", "<i4"), ("n_model", "<i4"),
                      ("n_pix", "<i4"), ("peak_section", "<i4"), ("q_removed", "<i8"), ("removed", "<f8"), ("peak", "<f8")])
SUB_OK, SUB_BAD_SEGMENT, SUB_TOO_LONG, SUB_EMPTY = 0, 1, 2, 3
SUB_MAX_SMOOTH = 8


def make_sub_params(**params):
    """lfdmi_default_sub_params with the given fields replaced (unknown names raise)."""
    return _make_params(SubParamsStruct, "lfdmi_default_sub_params", "subtraction", params)


class RadonParamsStruct(C.Structure):
    """lfdmi_radon_params (include/lfdmi.h: faint-trail search)."""
    _fields_ = [("bin", C.c_int32), ("min_len", C.c_int32), ("clip", C.c_float), ("threshold", C.c_float)]


class RadonResult(C.Structure):
    """lfdmi_radon_result: one record per frame of lfdmi_radon_search."""
    _fields_ = [("status", C.c_int32), ("found", C.c_int32), ("q", C.c_int32), ("y0", C.c_int32), ("s", C.c_int32),
                ("n_pix", C.c_int32), ("sum", C.c_float), ("snr", C.c_float),
                ("x1", C.c_double), ("y1", C.c_double), ("x2", C.c_double), ("y2", C.c_double), ("rho", C.c_double), ("theta", C.c_double)]


RADON_DTYPE = np.dtype([("status", "<i4"), ("found", "<i4"), ("q", "<i4"), ("y0", "<i4"), ("s", "<i4"), ("n_pix", "<i4"),
                        ("sum", "<f4"), ("snr", "<f4"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"),
                        ("rho", "<f8"), ("theta", "<f8")])
RADON_OK, RADON_NO_LINE = 0, 1


class RadonLinesParamsStruct(C.Structure):
    """lfdmi_radon_lines_params (include/lfdmi.h: faint-trail search, steps 7 - 9)."""
    _fields_ = [("max_lines", C.c_int32), ("peel_halfwidth", C.c_int32), ("min_seg", C.c_int32)]


class RadonLine(C.Structure):
    """lfdmi_radon_line: one record per frame and round of lfdmi_radon_search_lines."""
    _fields_ = RadonResult._fields_ + [("c1", C.c_int32), ("c2", C.c_int32), ("seg_n_pix", C.c_int32), ("pad", C.c_int32),
                                       ("seg_sum", C.c_float), ("seg_snr", C.c_float),
                                       ("ex1", C.c_double), ("ey1", C.c_double), ("ex2", C.c_double), ("ey2", C.c_double)]


RADON_LINE_DTYPE = np.dtype(RADON_DTYPE.descr + [("c1", "<i4"), ("c2", "<i4"), ("seg_n_pix", "<i4"), ("pad", "<i4"),
                                                 ("seg_sum", "<f4"), ("seg_snr", "<f4"),
                                                 ("ex1", "<f8"), ("ey1", "<f8"), ("ex2", "<f8"), ("ey2", "<f8")])
RADON_MAX_LINES = 8


def make_radon_lines_params(**params):
    """lfdmi_default_radon_lines_params with the given fields replaced (unknown names raise)."""
    return _make_params(RadonLinesParamsStruct, "lfdmi_default_radon_lines_params", "radon lines", params)


class RadonShortParamsStruct(C.Structure):
    """lfdmi_radon_short_params (include/lfdmi.h: faint-trail search, steps 10 - 12)."""
    _fields_ = [("min_strip", C.c_int32), ("max_lines", C.c_int32), ("peel_halfwidth", C.c_int32), ("min_seg", C.c_int32),
                ("short_threshold", C.c_float), ("pad", C.c_int32)]


class RadonShort(C.Structure):
    """lfdmi_radon_short: one record per frame and round of lfdmi_radon_search_short."""
    _fields_ = RadonLine._fields_ + [("level", C.c_int32), ("strip", C.c_int32), ("ys", C.c_int32), ("ss", C.c_int32)]


RADON_SHORT_DTYPE = np.dtype(RADON_LINE_DTYPE.descr + [("level", "<i4"), ("strip", "<i4"), ("ys", "<i4"), ("ss", "<i4")])


def make_radon_short_params(**params):
    """lfdmi_default_radon_short_params with the given fields replaced (unknown names raise)."""
    return _make_params(RadonShortParamsStruct, "lfdmi_default_radon_short_params", "radon short", params)


class RadonWideParamsStruct(C.Structure):
    """lfdmi_radon_wide_params (include/lfdmi.h: faint-trail search, steps 13 - 16)."""
    _fields_ = [("max_width", C.c_int32), ("max_lines", C.c_int32), ("peel_halfwidth", C.c_int32), ("min_seg", C.c_int32),
                ("wide_threshold", C.c_float), ("pad", C.c_int32)]


class RadonWide(C.Structure):
    """lfdmi_radon_wide: one record per frame and round of lfdmi_radon_search_wide."""
    _fields_ = RadonLine._fields_ + [("width", C.c_int32), ("pad2", C.c_int32), ("width_px", C.c_double)]


RADON_WIDE_DTYPE = np.dtype(RADON_LINE_DTYPE.descr + [("width", "<i4"), ("pad2", "<i4"), ("width_px", "<f8")])
RADON_MAX_WIDTH = 16
RADON_NULL_LINES, RADON_NULL_SHORT, RADON_NULL_WIDE = 0, 1, 2
RADON_NULL_MAX = 64
RADON_NULL_KINDS = {"lines": RADON_NULL_LINES, "short": RADON_NULL_SHORT, "wide": RADON_NULL_WIDE}
RADON_NULL_SCRAMBLE, RADON_NULL_SIGNFLIP, RADON_NULL_ROWSHIFT, RADON_NULL_COLSHIFT = 0, 1, 2, 3
RADON_NULL_SCHEMES = {"scramble": RADON_NULL_SCRAMBLE, "signflip": RADON_NULL_SIGNFLIP, "rowshift": RADON_NULL_ROWSHIFT,
                      "colshift": RADON_NULL_COLSHIFT}


class RadonPeel(C.Structure):
    """lfdmi_radon_peel: a line whose band lfdmi_radon_null_scheme blots before it searches (width 0: no line in this place)."""
    _fields_ = [("q", C.c_int32), ("y0", C.c_int32), ("s", C.c_int32), ("width", C.c_int32)]


RADON_PEEL_DTYPE = np.dtype([("q", "<i4"), ("y0", "<i4"), ("s", "<i4"), ("width", "<i4")])


def make_radon_wide_params(**params):
    """lfdmi_default_radon_wide_params with the given fields replaced (unknown names raise)."""
    return _make_params(RadonWideParamsStruct, "lfdmi_default_radon_wide_params", "radon wide", params)


class StackParamsStruct(C.Structure):
    """lfdmi_stack_params (include/lfdmi.h: stacked cross-sections)."""
    _fields_ = [("wing", C.c_int32), ("n_iter", C.c_int32), ("min_cols", C.c_int32), ("clip", C.c_float),
                ("prof_half", C.c_double), ("step", C.c_double), ("box", C.c_double), ("max_shift", C.c_double),
                ("k_sig", C.c_double), ("k_ref", C.c_double), ("pixscale", C.c_double)]


# lfdmi_stack_segment: one record per segment of lfdmi_stack_profiles
STACK_SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("pad", "<i4"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8")])
# lfdmi_stack: its result
STACK_DTYPE = np.dtype([("status", "<i4"), ("n_col", "<i4"), ("min_valid", "<i4"), ("n_pass", "<i4"),
                        ("rho", "<f8"), ("theta", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"),
                        ("background", "<f8"), ("noise", "<f8"), ("peak", "<f8"),
                        ("fwhm", "<f8"), ("fwhm_arcsec", "<f8"), ("depth", "<f8"),
                        ("flux", "<f8"), ("flux_err", "<f8"), ("snr", "<f8"), ("shift", "<f8"), ("tilt", "<f8")])
STACK_OK, STACK_BAD_SEGMENT, STACK_TOO_SHORT, STACK_TOO_FAINT = 0, 1, 2, 3
STACK_MAX_HALF = 40.0


def make_stack_params(**params):
    """lfdmi_default_stack_params with the given fields replaced (unknown names raise)."""
    return _make_params(StackParamsStruct, "lfdmi_default_stack_params", "stack", params)


def stack_bins(p):
    """2K+1 profile bins of a StackParamsStruct"""
    return 2 * int(round(p.prof_half / p.step)) + 1


class StarsParamsStruct(C.Structure):
    """lfdmi_stars_params (include/lfdmi.h: source finder)."""
    _fields_ = [("k_det", C.c_double), ("k_edge", C.c_double), ("edge_frac", C.c_double),
                ("sep", C.c_int32), ("r_max", C.c_int32), ("max_obj", C.c_int32)]


# lfdmi_star: one record per source of lfdmi_find_stars; lfdmi_stars_frame: one per frame
STAR_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("rad", "<i4"), ("flags", "<i4"),
                       ("s_peak", "<f4"), ("flux", "<f4"), ("xc", "<f4"), ("yc", "<f4")])
STARS_FRAME_DTYPE = np.dtype([("status", "<i4"), ("n_found", "<i4"), ("n_out", "<i4")])
STARS_OK, STARS_TRUNCATED = 0, 1
STAR_EXTENDED, STAR_EDGE = 1, 2
STARS_MAX_OBJ = 1048576
CATALOG_KEYS5 = ("ROWC", "COLC", "PSFMAG", "PETROTH90")


def make_stars_params(**params):
    """lfdmi_default_stars_params with the given fields replaced (unknown names raise)."""
    return _make_params(StarsParamsStruct, "lfdmi_default_stars_params", "stars", params)


class PsfParamsStruct(C.Structure):
    """lfdmi_psf_params (include/lfdmi.h: frame seeing)."""
    _fields_ = [("k_peak", C.c_double), ("e_max", C.c_double), ("sat", C.c_double),
                ("win", C.c_int32), ("gap", C.c_int32), ("ring", C.c_int32), ("iso", C.c_int32), ("rad_max", C.c_int32),
                ("min_stars", C.c_int32), ("max_used", C.c_int32), ("pad", C.c_int32)]


# lfdmi_psf_star: one packed record per OK star of lfdmi_measure_seeing; lfdmi_seeing_frame: one per frame
PSF_STAR_DTYPE = np.dtype([("index", "<i4"), ("n_ring", "<i4"), ("Q0", "<i8"), ("Qx", "<i8"), ("Qy", "<i8"), ("Qxx", "<i8"),
                           ("Qyy", "<i8"), ("Qxy", "<i8"), ("Q_ring", "<i8")])
SEEING_FRAME_DTYPE = np.dtype([("status", "<i4"), ("n_cand", "<i4"), ("n_ok", "<i4"), ("n_packed", "<i4"), ("n_used", "<i4"),
                               ("n_not_candidate", "<i4"), ("n_clipped", "<i4"), ("n_crowded", "<i4"), ("n_bad_pixel", "<i4"),
                               ("pad", "<i4"), ("fwhm_px", "<f8"), ("scatter", "<f8"), ("ell", "<f8")])
PSF_OK, PSF_NOT_CANDIDATE, PSF_CLIPPED, PSF_CROWDED, PSF_BAD_PIXEL = 0, 1, 2, 3, 4
SEEING_OK, SEEING_FEW = 0, 1
PSF_MAX_SAT = 4096.0
PSF_MAX_USED = 1024


def make_psf_params(**params):
    """lfdmi_default_psf_params with the given fields replaced (unknown names raise)."""
    return _make_params(PsfParamsStruct, "lfdmi_default_psf_params", "psf", params)


class RoundsParamsStruct(C.Structure):
    """lfdmi_rounds_params (include/lfdmi.h: detection rounds)."""
    _fields_ = [("max_trails", C.c_int32), ("pad", C.c_int32), ("half", C.c_double), ("dup_dist", C.c_double)]


ROUNDS_MAX_TRAILS = 8


def make_rounds_params(**params):
    """lfdmi_rounds_params: the library's defaults with the given fields replaced (unknown names raise)"""
    return _make_params(RoundsParamsStruct, "lfdmi_default_rounds_params", "rounds", params)


class PreviewParamsStruct(C.Structure):
    """lfdmi_preview_params (include/lfdmi.h: frame previews)."""
    _fields_ = [("bin", C.c_int32), ("mode", C.c_int32), ("lo_ppm", C.c_int32), ("hi_ppm", C.c_int32)]


# lfdmi_preview_frame: one record per frame of lfdmi_frame_previews
PREVIEW_FRAME_DTYPE = np.dtype([("status", "<i4"), ("n_cells", "<i4"), ("n_empty", "<i4"), ("pad", "<i4"),
                                ("lo", "<i8"), ("hi", "<i8"), ("lo_f", "<f8"), ("hi_f", "<f8")])
PREVIEW_RANK, PREVIEW_GIVEN = 0, 1
PREVIEW_MODES = ("rank", "given")
PREVIEW_OK, PREVIEW_FLAT, PREVIEW_EMPTY = 0, 1, 2
PREVIEW_LUT = 4096
PREVIEW_BINS = (1, 2, 4, 8, 16)
PREVIEW_EMPTY_CELL = -2 ** 63


def _preview_mode(k, v):
    if k == "mode" and isinstance(v, str):
        if v not in PREVIEW_MODES:
            raise ValueError(f"unknown preview mode {v!r}")
        return PREVIEW_MODES.index(v)
    return v


def make_preview_params(**params):
    """lfdmi_default_preview_params with the given fields replaced (unknown names raise; mode: a name of PREVIEW_MODES or its code)."""
    return _make_params(PreviewParamsStruct, "lfdmi_default_preview_params", "preview", params, _preview_mode)


class StreakParamsStruct(C.Structure):
    """lfdmi_streak_params (include/lfdmi.h: short-streak search)."""
    _fields_ = [("bin", C.c_int32), ("length", C.c_int32), ("max_streaks", C.c_int32), ("peel_halfwidth", C.c_int32),
                ("clip", C.c_float), ("threshold", C.c_float)]


class Streak(C.Structure):
    """lfdmi_streak: one record per frame and round of lfdmi_streak_search."""
    _fields_ = [("status", C.c_int32), ("found", C.c_int32), ("q", C.c_int32), ("s", C.c_int32), ("r0", C.c_int32), ("c0", C.c_int32),
                ("n_pix", C.c_int32), ("sum", C.c_float), ("snr", C.c_float), ("pad", C.c_int32),
                ("x1", C.c_double), ("y1", C.c_double), ("x2", C.c_double), ("y2", C.c_double), ("rho", C.c_double), ("theta", C.c_double)]


STREAK_DTYPE = np.dtype([("status", "<i4"), ("found", "<i4"), ("q", "<i4"), ("s", "<i4"), ("r0", "<i4"), ("c0", "<i4"), ("n_pix", "<i4"),
                         ("sum", "<f4"), ("snr", "<f4"), ("pad", "<i4"), ("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8"),
                         ("rho", "<f8"), ("theta", "<f8")])
STREAK_OK, STREAK_NONE = 0, 1
STREAK_MAX_STREAKS = 8


def make_streak_params(**params):
    """lfdmi_default_streak_params with the given fields replaced (unknown names raise)."""
    return _make_params(StreakParamsStruct, "lfdmi_default_streak_params", "streak", params)


def streak_tile():
    """(rows, columns) of anchors a workgroup of k_streak_search owns"""
    r, c = C.c_int32(), C.c_int32()
    lib().lfdmi_streak_tile(C.byref(r), C.byref(c))
    return r.value, c.value


def make_radon_params(**params):
    """lfdmi_default_radon_params with the given fields replaced (unknown names raise)."""
    return _make_params(RadonParamsStruct, "lfdmi_default_radon_params", "radon", params)


_lib = None


def lib():
    """Load liblfdmi.so or fail loudly (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C lfd_amd/csrc` "
                              "(or `python -c 'import __graft_entry__ as g; g.build()'`)")
        _lib = C.CDLL(LIB_PATH)
        _lib.lfdmi_last_error.restype = C.c_char_p
        _lib.lfdmi_last_error.argtypes = [C.c_void_p]
        _lib.lfdmi_ctx_destroy.restype = None
        _lib.lfdmi_ctx_destroy.argtypes = [C.c_void_p]
        _lib.lfdmi_hough_dims.restype = None
        _lib.lfdmi_default_caps.restype = None
        _lib.lfdmi_ctx_bytes.restype = C.c_int64
        _lib.lfdmi_ctx_bytes.argtypes = [C.c_void_p]
        _lib.lfdmi_spill_count.restype = C.c_int64
        _lib.lfdmi_spill_count.argtypes = [C.c_void_p]
        _lib.lfdmi_timing_name.restype = C.c_char_p
        _lib.lfdmi_bz2_find_blocks.restype = C.c_int64
        _lib.lfdmi_bz2_find_blocks.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64]
        _lib.lfdmi_bz2_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _lib.lfdmi_bz2_destroy.restype = None
        _lib.lfdmi_bz2_destroy.argtypes = [C.c_void_p]
        _lib.lfdmi_bz2_last_error.restype = C.c_char_p
        _lib.lfdmi_bz2_last_error.argtypes = [C.c_void_p]
        _lib.lfdmi_bz2_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64,
                                                C.c_void_p, C.c_void_p]
        _lib.lfdmi_bz2_fetch.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]
        _lib.lfdmi_bz2_fetch_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _lib.lfdmi_bz2_timings.argtypes = [C.c_void_p, C.c_void_p]
        _lib.lfdmi_bz2_frames.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
        _lib.lfdmi_bz2_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint64]
        _lib.lfdmi_default_defocus_params.restype = None
        _lib.lfdmi_default_defocus_params.argtypes = [C.c_void_p]
        _lib.lfdmi_defocus_bank_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.lfdmi_defocus_bank_destroy.restype = None
        _lib.lfdmi_defocus_bank_destroy.argtypes = [C.c_void_p]
        _lib.lfdmi_defocus_bank_dims.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_defocus_bank_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_fit_defocus.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
        _lib.lfdmi_default_sky_params.restype = None
        _lib.lfdmi_default_sky_params.argtypes = [C.c_void_p]
        _lib.lfdmi_sky_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.lfdmi_sky_destroy.restype = None
        _lib.lfdmi_sky_destroy.argtypes = [C.c_void_p]
        _lib.lfdmi_sky_dims.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_sky_frames.restype = C.c_void_p
        _lib.lfdmi_sky_frames.argtypes = [C.c_void_p]
        _lib.lfdmi_sky_normalize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_inject_trails.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int]
        _lib.lfdmi_default_mask_params.restype = None
        _lib.lfdmi_default_mask_params.argtypes = [C.c_void_p]
        _lib.lfdmi_mask_trails.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.lfdmi_default_lc_params.restype = None
        _lib.lfdmi_default_lc_params.argtypes = [C.c_void_p]
        _lib.lfdmi_light_curves.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _lib.lfdmi_default_strip_params.restype = None
        _lib.lfdmi_default_strip_params.argtypes = [C.c_void_p]
        _lib.lfdmi_trail_strips.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        _lib.lfdmi_default_sub_params.restype = None
        _lib.lfdmi_default_sub_params.argtypes = [C.c_void_p]
        _lib.lfdmi_subtract_trails.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _lib.lfdmi_default_radon_params.restype = None
        _lib.lfdmi_default_radon_params.argtypes = [C.c_void_p]
        _lib.lfdmi_radon_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        _lib.lfdmi_radon_destroy.restype = None
        _lib.lfdmi_radon_destroy.argtypes = [C.c_void_p]
        _lib.lfdmi_radon_dims.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_radon_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.lfdmi_default_radon_lines_params.restype = None
        _lib.lfdmi_default_radon_lines_params.argtypes = [C.c_void_p]
        _lib.lfdmi_radon_search_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        _lib.lfdmi_default_radon_short_params.restype = None
        _lib.lfdmi_default_radon_short_params.argtypes = [C.c_void_p]
        _lib.lfdmi_default_radon_wide_params.restype = None
        _lib.lfdmi_default_radon_wide_params.argtypes = [C.c_void_p]
        _lib.lfdmi_radon_search_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_radon_null.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.lfdmi_radon_null_scheme.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.lfdmi_radon_search_short.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_default_stack_params.restype = None
        _lib.lfdmi_default_stack_params.argtypes = [C.c_void_p]
        _lib.lfdmi_stack_profiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_default_stars_params.restype = None
        _lib.lfdmi_default_stars_params.argtypes = [C.c_void_p]
        _lib.lfdmi_find_stars.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p]
        _lib.lfdmi_stars_catalog.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        _lib.lfdmi_default_psf_params.restype = None
        _lib.lfdmi_default_psf_params.argtypes = [C.c_void_p]
        _lib.lfdmi_measure_seeing.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lfdmi_default_rounds_params.restype = None
        _lib.lfdmi_default_rounds_params.argtypes = [C.c_void_p]
        _lib.lfdmi_detect_rounds.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _lib.lfdmi_default_preview_params.restype = None
        _lib.lfdmi_default_preview_params.argtypes = [C.c_void_p]
        _lib.lfdmi_frame_previews.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.lfdmi_default_streak_params.restype = None
        _lib.lfdmi_default_streak_params.argtypes = [C.c_void_p]
        _lib.lfdmi_streak_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
        _lib.lfdmi_streak_tile.restype = None
        _lib.lfdmi_streak_tile.argtypes = [C.c_void_p, C.c_void_p]
        _lib.lfdmi_debug_unit_limits.argtypes = [C.c_void_p, C.c_void_p]
        _lib.lfdmi_debug_unit_split.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return _lib


def _is_dev(a):
    return hasattr(a, "data_ptr")


def _ptr(a):
    if a is None:
        return None
    if _is_dev(a):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _dtype_code(a):
    name = str(a.dtype).replace("torch.", "")
    try:
        return {"uint8": U8, "float32": F32, "float64": F64}[name]
    except KeyError:
        raise TypeError(f"unsupported image dtype {a.dtype}") from None


def _sigma(sigma, n):
    """None, a number or n values -> None or n float32 values"""
    if sigma is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, np.float32), (n,)))


def make_params(d, dim=False):
    """dict with the reference's key names -> (Params struct, objects to keep alive)."""
    dk = np.ascontiguousarray(d["dilateKernel"], np.uint8)
    if dk.ndim != 2:
        raise ValueError("dilateKernel must be a 2-d array")
    keep = [dk]
    p = Params()
    p.lwTresh = float(d["lwTresh"])
    p.thetaTresh = float(d["thetaTresh"])
    p.lineSetTresh = float(d["lineSetTresh"])
    p.dro = float(d["dro"])
    p.minAreaRectMinLen = float(d["minAreaRectMinLen"])
    p.houghMethod = float(d["houghMethod"])
    p.nlinesInSet = int(d["nlinesInSet"])
    p.contoursMode = int(d["contoursMode"])
    p.contoursMethod = int(d["contoursMethod"])
    p.dilate_kh, p.dilate_kw = dk.shape
    p.dilateKernel = dk.ctypes.data
    if dim:
        ek = np.ascontiguousarray(d["erodeKernel"], np.uint8)
        if ek.ndim != 2:
            raise ValueError("erodeKernel must be a 2-d array")
        keep.append(ek)
        p.erode_kh, p.erode_kw = ek.shape
        p.erodeKernel = ek.ctypes.data
        p.minFlux = float(d["minFlux"])
        p.addFlux = float(d["addFlux"])
    p.gaussKernel = int(d.get("gaussKernel", 0) or 0)       # optional smoothing of Canny's input; off in the reference
    p.gaussSigma = float(d.get("gaussSigma", 0.0) or 0.0)
    return p, keep


def make_rs_params(filter, defaultxy, filter_caps, maxxy, pixscale, magcount, maxmagdiff, **_):
    return RsParams(int(defaultxy), int(maxxy), int(magcount), float(pixscale), float(maxmagdiff),
                    float(filter_caps[filter]), "ugriz".index(filter))


class PinnedBuffer:
    """``nbytes`` of page-locked host memory from lfdmi_host_alloc; ``.array`` is a uint8 numpy view (take ``.view('>f4')``
    slices of it for frames).  Freed by ``close()`` / garbage collection; the views must not be used afterwards."""

    def __init__(self, ctx, nbytes):
        self._lib = ctx._lib
        self._p = C.c_void_p()
        self.nbytes = int(nbytes)
        self._lib.lfdmi_host_alloc.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        ctx._chk(self._lib.lfdmi_host_alloc(ctx._h, C.c_uint64(self.nbytes), C.byref(self._p)))
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self._p.value))

    def close(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            self.array = None
            self._lib.lfdmi_host_free.argtypes = [C.c_void_p, C.c_void_p]
            self._lib.lfdmi_host_free(None, p)

    __del__ = close


BZ2_STATUS = {0: "ok", 1: "no block magic", 2: "randomised block", 3: "bad block header", 4: "bad compressed data",
              5: "block length mismatch", 6: "bad origin pointer", 7: "CRC mismatch", 8: "BWT cycle shorter than the block",
              9: "larger than out_cap", 10: "not a sequence of bzip2 streams"}


class DeviceFrames:
    """n big-endian float32 frames (the data units of FITS images) in device memory that belongs to a ``Bz2Decoder``: what
    ``Context.detect_batch`` takes instead of an array when the frames were decompressed on the GPU and never left it."""

    def __init__(self, ptr, shape):
        self._ptr = int(ptr)
        self.shape = tuple(int(x) for x in shape)            # (n, h, w)

    def data_ptr(self):
        return self._ptr

    @property
    def frame_bytes(self):
        return self.shape[1] * self.shape[2] * 4

    def address_of(self, k):
        return self._ptr + int(k) * self.frame_bytes

    def slice(self, a, b):
        return DeviceFrames(self.address_of(a), (int(b) - int(a), self.shape[1], self.shape[2]))


class NativeDeviceFrames(DeviceFrames):
    """n native float32 frames in device memory that belongs to a ``Sky`` handle (its normalised output): taken as LFDMI_F32
    device frames by ``detect_batch``, ``process_multiscale`` and ``measure_trails``."""
    native = True
    dtype = "float32"

    def is_contiguous(self):
        return True

    def slice(self, a, b):
        return NativeDeviceFrames(self.address_of(a), (int(b) - int(a), self.shape[1], self.shape[2]))


class Bz2Decoder:
    """lfdmi_bz2_*: whole ``.bz2`` files decompressed on the GPU, many at once (include/lfdmi.h).  ``decode`` takes the
    compressed files as one uint8 array + offsets / lengths and returns (out_len, status, heads); the decompressed bytes stay on
    the device until the next ``decode`` and are copied out in ranges by ``fetch`` / ``fetch_many``.  A file whose status is not
    0 was NOT decoded (a broken block, trailing bytes, ...): decompress it on the host, as the reference does."""

    def __init__(self, device=0):
        self._lib = lib()
        self._h = C.c_void_p()
        rc = self._lib.lfdmi_bz2_create(int(device), C.byref(self._h))
        if rc:
            raise NativeError(rc, "lfdmi_bz2_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.lfdmi_bz2_destroy(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc:
            raise NativeError(rc, (self._lib.lfdmi_bz2_last_error(self._h) or b"").decode())

    def decode(self, src, offsets, lengths, out_cap, head_bytes=0):
        src = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lengths, np.uint64)
        n = len(off)
        if n == 0 or len(ln) != n or (n and int((off + ln).max()) > src.size):
            raise ValueError("Bz2Decoder.decode: offsets / lengths do not fit the source array")
        out_len = np.zeros(n, np.uint64)
        status = np.zeros(n, np.int32)
        heads = np.zeros((n, int(head_bytes)), np.uint8) if head_bytes else None
        self._chk(self._lib.lfdmi_bz2_decode_batch(self._h, _ptr(src), _ptr(off), _ptr(ln), n, C.c_uint64(int(out_cap)),
                                                   _ptr(heads), C.c_uint64(int(head_bytes)), _ptr(out_len), _ptr(status)))
        return out_len, status, heads

    def fetch(self, i, offset, nbytes, dst=None):
        """Bytes [offset, offset + nbytes) of decompressed file i into ``dst`` (a uint8 numpy array / torch CUDA tensor; a new
        numpy array if None)."""
        if dst is None:
            dst = np.empty(int(nbytes), np.uint8)
        self._chk(self._lib.lfdmi_bz2_fetch(self._h, int(i), C.c_uint64(int(offset)), C.c_uint64(int(nbytes)), _ptr(dst),
                                            DEVICE if _is_dev(dst) else HOST))
        return dst

    def fetch_many(self, files, offsets, nbytes, dsts):
        """One range per entry, all copies queued before one wait.  dsts: numpy arrays, torch CUDA tensors, or plain integers =
        device addresses (``DeviceFrames.address_of``), all of one kind."""
        n = len(files)
        if n == 0:
            return
        f = np.ascontiguousarray(files, np.int32)
        o = np.ascontiguousarray(offsets, np.uint64)
        b = np.ascontiguousarray(nbytes, np.uint64)
        on_dev = isinstance(dsts[0], int) or _is_dev(dsts[0])
        ptrs = (C.c_void_p * n)(*[C.c_void_p(d) if isinstance(d, int) else _ptr(d) for d in dsts])
        self._chk(self._lib.lfdmi_bz2_fetch_many(self._h, n, _ptr(f), _ptr(o), _ptr(b), ptrs, DEVICE if on_dev else HOST))

    def frames(self, which, n, h, w):
        """The handle's device buffer ``which`` (0 / 1), at least n frames of h x w float32 large, as ``DeviceFrames``."""
        p = C.c_void_p()
        self._chk(self._lib.lfdmi_bz2_frames(self._h, int(which), C.c_uint64(int(n) * int(h) * int(w) * 4), C.byref(p)))
        return DeviceFrames(p.value, (n, h, w))

    def reserve(self, n_files, n_blocks, out_cap, compressed_bytes=0):
        """Allocate the decoder's tables now (optional; otherwise inside the first ``decode``)."""
        self._chk(self._lib.lfdmi_bz2_reserve(self._h, int(n_files), int(n_blocks), C.c_uint64(int(out_cap)), C.c_uint64(int(compressed_bytes))))

    def timings(self):
        ms = np.zeros(5, np.float32)
        self._chk(self._lib.lfdmi_bz2_timings(self._h, _ptr(ms)))
        return dict(zip(("upload+magics", "huffman+mtf", "sort", "walk", "rle+crc+out"), (float(x) for x in ms)))


class Pending:
    """A call in flight on a ``Context`` (``detect_batch_begin`` / ``process_multiscale_begin``).  It holds every object the
    library reads until the call ends (ctypes structs, params, catalogue arrays, converted frames, rhos) and the result array
    the records land in.  ``result()`` ends the context's calls in FIFO order up to and including this one."""

    def __init__(self, ctx, res, keep, squeeze=False):
        self._ctx, self._res, self._keep, self._squeeze = ctx, res, keep, squeeze
        self._done, self._err = False, None

    def done(self):
        return self._done

    def _finish(self, err):
        self._done, self._err, self._keep = True, err, None

    def result(self):
        while not self._done:
            self._ctx._end_oldest()
        if self._err is not None:
            raise self._err
        return self._res[:, 0] if self._squeeze else self._res


class Context:
    """One GPU, one HIP stream, workspace for ``max_inflight`` frames of up to max_h x max_w."""

    def __init__(self, device=0, max_h=1489, max_w=2048, max_inflight=8, caps=None):
        """caps: None = the library's default table capacities (frames that need more are re-run through a
        worst-case workspace inside the library); "worst" = every table at its theoretical maximum; or a dict
        with any of run_cap / key_cap / slot_cap / list_cap / peak_cap / min_rho (others keep their defaults)."""
        self._h = C.c_void_p()
        self._lib = lib()
        if caps is None:
            rc = self._lib.lfdmi_ctx_create(int(device), int(max_h), int(max_w), int(max_inflight),
                                            C.byref(self._h))
        else:
            c = Caps()
            if caps != "worst":
                self._lib.lfdmi_default_caps(int(max_h), int(max_w), C.byref(c))
                for k, v in dict(caps).items():
                    setattr(c, k, v)
            rc = self._lib.lfdmi_ctx_create_sized(int(device), int(max_h), int(max_w), int(max_inflight),
                                                  C.byref(c), C.byref(self._h))
        if rc:
            msg = self._lib.lfdmi_last_error(self._h).decode() if self._h else "context creation failed"
            h, self._h = self._h, C.c_void_p()
            if h:
                self._lib.lfdmi_ctx_destroy(h)
            raise NativeError(rc, msg)
        self.device, self.max_h, self.max_w, self.max_inflight = device, max_h, max_w, max_inflight
        self._inflight = []                                  # Pending calls, oldest first

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            while getattr(self, "_inflight", None):          # (calls in flight end first: their results stay readable)
                self._end_oldest()
            for b in list(getattr(self, "_banks", ())):       # defocus banks of this context close with it
                b.close()
            for k in list(getattr(self, "_skies", ())):       # and so do its sky and radon handles
                k.close()
            self._lib.lfdmi_debug_unit_limits(h, None)       # (forgets what debug_unit_limits / a unit call noted beside the context)
            self._h = None
            self._lib.lfdmi_ctx_destroy(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc:
            raise NativeError(rc, self._lib.lfdmi_last_error(self._h).decode())

    def workspace_bytes(self):
        """Device bytes of the workspace (worst-case spill workspace included once it exists)."""
        return int(self._lib.lfdmi_ctx_bytes(self._h))

    def spill_count(self):
        """Frames this context has re-run through its worst-case workspace."""
        return int(self._lib.lfdmi_spill_count(self._h))

    def set_stream(self, stream_handle):
        self._chk(self._lib.lfdmi_set_stream(self._h, C.c_void_p(stream_handle or 0)))

    STAT_NAMES = ("spilled_frames", "scan_giveups", "general_reruns", "general_chunks", "chunks", "cap_growths", "scan_fused_on")

    def stats(self):
        """lfdmi_get_stats as a dict: what the context did besides the fast path (never changes a result, always costs time)."""
        out = np.zeros(len(self.STAT_NAMES), np.int64)
        self._chk(self._lib.lfdmi_get_stats(self._h, _ptr(out), len(out)))
        return dict(zip(self.STAT_NAMES, (int(v) for v in out)))

    def debug_trig(self, y, x):
        """(angle_deg, cos/2, sin/2) float32 as the rectangle kernels compute them from atan2(y, x) (developer check)."""
        y = np.ascontiguousarray(y, np.float64)
        x = np.ascontiguousarray(x, np.float64)
        n = y.size
        out = [np.zeros(n, np.float32) for _ in range(3)]
        self._chk(self._lib.lfdmi_debug_trig(self._h, n, _ptr(y), _ptr(x), *[_ptr(o) for o in out]))
        return out

    def debug_tail(self, h1, n1, h2, n2, navg, dro, thetaTresh, lineSetTresh, which, shape):
        """The tail of a pass on line sets given from outside: the device's check_theta (k_finalize) and the library's host-side
        dictify_hough, as detect_batch runs them.  h1 / h2: (n, kmax, 2) float32, n1 / n2: lines per set -> record array."""
        h1 = np.ascontiguousarray(h1, np.float32)
        h2 = np.ascontiguousarray(h2, np.float32)
        n1 = np.ascontiguousarray(n1, np.int32)
        n2 = np.ascontiguousarray(n2, np.int32)
        n, kmax = h1.shape[0], h1.shape[1]
        assert h2.shape == h1.shape and n1.shape == (n,) and n2.shape == (n,)
        out = np.zeros(n, RESULT_DTYPE)
        self._chk(self._lib.lfdmi_debug_tail(self._h, n, kmax, _ptr(h1), _ptr(n1), _ptr(h2), _ptr(n2), int(navg), C.c_double(dro),
                                             C.c_double(thetaTresh), C.c_double(lineSetTresh), int(which), int(shape[0]), int(shape[1]),
                                             _ptr(out)))
        return out

    def debug_fail_chunk(self, chunk):
        """Developer hook: the next detect_batch fails (ERR_ARG) at the top of chunk ``chunk`` (tests of the error path)."""
        self._chk(self._lib.lfdmi_debug_fail_chunk(self._h, int(chunk)))

    def debug_unit_limits(self, forget=False, **limits):
        """Developer hook (tests of the measurement units' chunk loops): lower the limits that split a unit's call on this
        context -- list_pairs, stage_bytes, cell_bytes, render_blocks, stars_rec_bytes, stack_part_bytes (include/lfdmi.h:
        lfdmi_debug_unit_limits).  A limit that is not named, or 0, is at its compiled default; no argument restores them all.
        From the first call of this or of ``debug_unit_split`` on, the context's unit calls record their split.
        A value can only lower a limit; a negative one is refused (ERR_ARG).  ``forget=True`` passes NULL: every default again
        and no split recorded any more, as on a context that never called this (``close`` does it)."""
        if forget:
            if limits:
                raise TypeError("debug_unit_limits: forget=True takes no limit")
            self._chk(self._lib.lfdmi_debug_unit_limits(self._h, None))
            return
        lim = UnitLimits()                                   # (zeros: every default, and the split goes on being recorded)
        for k, v in limits.items():
            if k not in dict(UnitLimits._fields_):
                raise TypeError(f"debug_unit_limits: unknown limit {k!r}")
            setattr(lim, k, int(v))
        self._chk(self._lib.lfdmi_debug_unit_limits(self._h, C.byref(lim)))

    def debug_unit_split(self):
        """How the last measurement unit call on this context was split: a dict of ``chunks`` (of jobs; find_stars: of frames;
        stack_profiles: groups of frames), ``batches`` (trail_strips' batches of cells), ``grid`` (the largest grid of persistent
        blocks) and ``launches`` (stack_profiles: of the first pass of the first group); 0 where the unit has no such count."""
        out = np.zeros(len(UNIT_SPLIT_NAMES), np.int64)
        self._chk(self._lib.lfdmi_debug_unit_split(self._h, _ptr(out), len(out)))
        return dict(zip(UNIT_SPLIT_NAMES, (int(v) for v in out)))

    def set_stage_images(self, mode):
        """Which calls keep the 8-bit stage images for get_stage: -1 the per-pass calls do and detect_batch does not
        (default), 0 none (batches), 1 all."""
        self._chk(self._lib.lfdmi_set_stage_images(self._h, int(mode)))

    def enable_timing(self, on=True):
        self._chk(self._lib.lfdmi_enable_timing(self._h, int(on)))

    def timing_select(self, names=None):
        """Bracket only the launches of the given timing slots (kernel names as in get_timing), or all (None)."""
        mask = 0
        if names:
            known = [self._lib.lfdmi_timing_name(i).decode() for i in range(self._lib.lfdmi_timing_slots())]
            for nm in ([names] if isinstance(names, str) else names):
                mask |= 1 << known.index(nm)
        self._lib.lfdmi_timing_select.argtypes = [C.c_void_p, C.c_uint64]
        self._chk(self._lib.lfdmi_timing_select(self._h, mask))

    def get_timing(self):
        """{kernel name: (total device ms, launches, frames worked on)} since enable_timing(True)."""
        k = self._lib.lfdmi_timing_slots()
        ms = (C.c_float * k)()
        n = (C.c_int32 * k)()
        u = (C.c_int64 * k)()
        self._chk(self._lib.lfdmi_get_timing(self._h, ms, n, u))
        return {self._lib.lfdmi_timing_name(i).decode(): (float(ms[i]), int(n[i]), int(u[i])) for i in range(k)}

    # -- helpers --------------------------------------------------------------------------
    @staticmethod
    def _batch(img, ndim_item=2):
        """-> (array with leading batch axis, n, h, w, squeeze?)"""
        if _is_dev(img):
            shp = tuple(img.shape)
            if not img.is_contiguous():
                raise ValueError("device tensors must be contiguous")
        else:
            img = np.ascontiguousarray(img)
            shp = img.shape
        if len(shp) == ndim_item:
            return img, 1, shp[0], shp[1], True
        if len(shp) == ndim_item + 1:
            return img, shp[0], shp[1], shp[2], False
        raise ValueError(f"expected a 2-d image or a 3-d batch, got shape {shp}")

    @staticmethod
    def _out_like(img, n, h, w, squeeze, dtype=np.uint8):
        if _is_dev(img):
            import torch
            tdt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32}[dtype]
            out = torch.empty((n, h, w), dtype=tdt, device=img.device)
        else:
            out = np.empty((n, h, w), dtype)
        return out

    # -- per-operator entry points ------------------------------------------------------------
    def prep_u8(self, img, mode, flip=False, minFlux=0.0, addFlux=0.0, want_hist=False):
        img, n, h, w, sq = self._batch(img)
        loc = DEVICE if _is_dev(img) else HOST
        out = self._out_like(img, n, h, w, sq)
        hist = None
        if want_hist:
            if loc == DEVICE:
                import torch
                hist = torch.empty((n, 256), dtype=torch.int32, device=img.device)
            else:
                hist = np.empty((n, 256), np.int32)
        self._chk(self._lib.lfdmi_prep_u8(self._h, _ptr(img), _dtype_code(img), n, h, w, int(flip),
                                          int(mode), C.c_double(minFlux), C.c_double(addFlux),
                                          _ptr(out), _ptr(hist), loc))
        out = out[0] if sq else out
        if want_hist:
            return out, (hist[0] if sq else hist)
        return out

    def equalize_hist(self, img):
        img, n, h, w, sq = self._batch(img)
        loc = DEVICE if _is_dev(img) else HOST
        out = self._out_like(img, n, h, w, sq)
        self._chk(self._lib.lfdmi_equalize_hist(self._h, _ptr(img), n, h, w, _ptr(out), loc))
        return out[0] if sq else out

    def _morph(self, fn, img, kernel):
        img, n, h, w, sq = self._batch(img)
        loc = DEVICE if _is_dev(img) else HOST
        k = np.ascontiguousarray(kernel, np.uint8)
        if k.ndim != 2:
            raise ValueError("kernel must be 2-d")
        out = self._out_like(img, n, h, w, sq)
        self._chk(fn(self._h, _ptr(img), n, h, w, _ptr(k), k.shape[0], k.shape[1], _ptr(out), loc))
        return out[0] if sq else out

    def dilate(self, img, kernel):
        return self._morph(self._lib.lfdmi_dilate, img, kernel)

    def erode(self, img, kernel):
        return self._morph(self._lib.lfdmi_erode, img, kernel)

    def gaussian_blur(self, img, ksize, sigma=0.0):
        img, n, h, w, sq = self._batch(img)
        loc = DEVICE if _is_dev(img) else HOST
        out = self._out_like(img, n, h, w, sq)
        self._chk(self._lib.lfdmi_gaussian_blur(self._h, _ptr(img), n, h, w, int(ksize), C.c_double(sigma), _ptr(out), loc))
        return out[0] if sq else out

    def canny(self, img, low=0.0, high=255.0):
        img, n, h, w, sq = self._batch(img)
        loc = DEVICE if _is_dev(img) else HOST
        out = self._out_like(img, n, h, w, sq)
        self._chk(self._lib.lfdmi_canny(self._h, _ptr(img), n, h, w, C.c_double(low), C.c_double(high),
                                        _ptr(out), loc))
        return out[0] if sq else out

    def fit_min_area_rect(self, img, contoursMode=1, contoursMethod=1, minAreaRectMinLen=1, lwTresh=5,
                          want_box=True):
        """-> (detection bool(s), box_img(s), n_boxes)"""
        img, n, h, w, sq = self._batch(img)
        if _is_dev(img):
            raise TypeError("fit_min_area_rect: pass numpy arrays (device outputs not wired in Python)")
        box = np.empty((n, h, w), np.uint8) if want_box else None
        det = np.zeros(n, np.int32)
        nb = np.zeros(n, np.int32)
        self._chk(self._lib.lfdmi_fit_min_area_rect(self._h, _ptr(img), n, h, w, int(contoursMode),
                                                    int(contoursMethod), C.c_double(minAreaRectMinLen),
                                                    C.c_double(lwTresh), _ptr(box), _ptr(det), _ptr(nb),
                                                    HOST))
        if sq:
            return bool(det[0]), (box[0] if want_box else None), int(nb[0])
        return det.astype(bool), box, nb

    def hough_dims(self, h, w, rho, theta=np.pi / 180):
        na, nr = C.c_int(), C.c_int()
        self._lib.lfdmi_hough_dims(int(h), int(w), C.c_double(rho), C.c_double(theta), C.byref(na), C.byref(nr))
        return na.value, nr.value

    def hough_lines(self, img, rho, theta=np.pi / 180, threshold=1, max_lines=None):
        """cv2.HoughLines layout per image: (n_lines, 1, 2) float32 or None; also total count."""
        img, n, h, w, sq = self._batch(img)
        if _is_dev(img):
            raise TypeError("hough_lines: pass numpy arrays")
        na, nr = self.hough_dims(h, w, rho, theta)
        cap = na * nr if max_lines is None else int(max_lines)
        lines = np.zeros((n, max(cap, 1), 2), np.float32)
        cnt = np.zeros(n, np.int32)
        self._chk(self._lib.lfdmi_hough_lines(self._h, _ptr(img), n, h, w, C.c_double(rho), C.c_double(theta),
                                              int(threshold), cap, _ptr(lines), _ptr(cnt), HOST))
        outs = []
        for i in range(n):
            k = min(int(cnt[i]), cap)
            outs.append(lines[i, :k].reshape(k, 1, 2).copy() if k else None)
        return (outs[0], int(cnt[0])) if sq else (outs, cnt)

    def hough_accum(self, img, rho, theta=np.pi / 180):
        img, n, h, w, sq = self._batch(img)
        na, nr = self.hough_dims(h, w, rho, theta)
        acc = np.zeros((n, na + 2, nr + 2), np.int32)
        self._chk(self._lib.lfdmi_hough_accum(self._h, _ptr(img), n, h, w, C.c_double(rho), C.c_double(theta),
                                              _ptr(acc), HOST))
        return acc[0] if sq else acc

    @staticmethod
    def _catalog(cat):
        """dict of stacked arrays (see synth.pack_catalogs) -> (Catalog struct, keep-alive list)"""
        if cat is None:
            return None, []
        dev = _is_dev(cat["ROWC"])
        if dev:
            arrs = {k: cat[k] for k in ("count", "ROWC", "COLC", "PSFMAG", "PETROTH90", "NOBSERVE", "NDETECT")}
        else:
            arrs = {"count": np.ascontiguousarray(cat["count"], np.int32)}
            for k in ("ROWC", "COLC", "PSFMAG", "PETROTH90"):
                arrs[k] = np.ascontiguousarray(cat[k], np.float32)
            for k in ("NOBSERVE", "NDETECT"):
                arrs[k] = np.ascontiguousarray(cat[k], np.int32)
        c = Catalog()
        c.max_obj = int(arrs["NOBSERVE"].shape[1])
        c.count = _ptr(arrs["count"]).value
        c.rowc = _ptr(arrs["ROWC"]).value
        c.colc = _ptr(arrs["COLC"]).value
        c.psfmag = _ptr(arrs["PSFMAG"]).value
        c.petro90 = _ptr(arrs["PETROTH90"]).value
        c.nobserve = _ptr(arrs["NOBSERVE"]).value
        c.ndetect = _ptr(arrs["NDETECT"]).value
        c.loc = DEVICE if dev else HOST
        return c, list(arrs.values())

    def remove_stars(self, img, cat, rs):
        """float32 frame(s), mutated in place like removestars.py:231."""
        b, n, h, w, sq = self._batch(img)
        if _dtype_code(b) != F32:
            raise TypeError("remove_stars needs float32 frames")
        if not _is_dev(img) and b is not img and not np.shares_memory(b, img):
            raise ValueError("remove_stars needs a C-contiguous array (it is modified in place)")
        c, keep = self._catalog(cat)
        self._chk(self._lib.lfdmi_remove_stars(self._h, _ptr(b), n, h, w, C.byref(c), C.byref(rs),
                                               DEVICE if _is_dev(b) else HOST))
        return img

    # -- whole passes -------------------------------------------------------------------------
    def _pass(self, fn, img, params, dim, flip, extra):
        img, n, h, w, sq = self._batch(img)
        loc = DEVICE if _is_dev(img) else HOST
        p, keep = make_params(params, dim=dim)
        res = np.zeros(n, RESULT_DTYPE)
        K = p.nlinesInSet
        le = np.zeros((n, K, 2), np.float32)
        lb = np.zeros((n, K, 2), np.float32)
        self._chk(fn(self._h, _ptr(img), _dtype_code(img), n, h, w, int(flip), *extra, C.byref(p), _ptr(res),
                     _ptr(le), _ptr(lb), loc))
        return (res[0], le[0], lb[0]) if sq else (res, le, lb)

    def process_bright(self, img, params, flip=False):
        return self._pass(self._lib.lfdmi_process_bright, img, params, False, flip, ())

    def process_dim(self, img, params, flip=False, after_bright=False):
        return self._pass(self._lib.lfdmi_process_dim, img, params, True, flip, (int(after_bright),))

    def process_multiscale(self, img, params, rhos, dim=True, flip=False, after_bright=False):
        """One pass with HoughLines evaluated at every rho of ``rhos``; returns a structured array
        [len(rhos), n] (or [len(rhos)] for a single image): row s == process_dim/bright with houghMethod=rhos[s]."""
        img, n, h, w, sq = self._batch(img)
        loc = DEVICE if _is_dev(img) else HOST
        p, keep = make_params(params, dim=dim)
        rh = (C.c_double * len(rhos))(*[float(r) for r in rhos])
        res = np.zeros((len(rhos), n), RESULT_DTYPE)
        self._chk(self._lib.lfdmi_process_multiscale(self._h, _ptr(img), _dtype_code(img), n, h, w, int(flip), int(dim),
                                                     int(after_bright), C.byref(p), len(rhos), rh, _ptr(res), loc))
        return res[:, 0] if sq else res

    def _frames(self, frames, pinned, what, contiguous=False, native_device=False):
        """The frames of detect_batch / detect_batch_begin / measure_trails -> (frames, dtype code, n, h, w, loc).
        ``DeviceFrames`` (decompressed on the device by Bz2Decoder.frames) are big-endian until ``detect_batch`` has swapped
        them in place (``native_device``); '>f4' numpy frames go as they are; float32 numpy / torch CUDA frames through
        ``_batch``, which copies a non-contiguous array (``contiguous``: refused instead)."""
        if isinstance(frames, DeviceFrames):
            n, h, w = frames.shape
            code = F32 if (native_device or getattr(frames, "native", False)) else F32_BE
        elif not _is_dev(frames) and isinstance(frames, np.ndarray) and frames.dtype == np.dtype(">f4"):
            if not frames.flags.c_contiguous:
                raise ValueError("big-endian frames must be C-contiguous")
            shp = frames.shape
            n, h, w = (1, *shp) if len(shp) == 2 else shp
            code = F32_BE
        else:
            if contiguous and not _is_dev(frames) and not (isinstance(frames, np.ndarray) and frames.flags.c_contiguous):
                raise ValueError("frames of a call in flight must be C-contiguous (they are used, and blotted, in place)")
            frames, n, h, w, sq = self._batch(frames)
            code = _dtype_code(frames)
            if code != F32:
                raise TypeError(f"{what} needs float32 frames")
        if pinned and _is_dev(frames):
            raise ValueError("pinned=True is for host arrays")
        return frames, code, n, h, w, DEVICE if _is_dev(frames) else (HOST_PINNED if pinned else HOST)

    def detect_batch(self, frames, params_bright, params_dim, cat=None, rs=None, pinned=False):
        """frames: float32 (n,h,w) numpy or torch-CUDA; returns a structured array of n results.

        numpy frames of dtype '>f4' (the raw data unit of a FITS image) are accepted as they are and byte-swapped on the
        device, ``DeviceFrames`` swapped in place there.  ``pinned=True``: the array lives in memory from ``PinnedBuffer``
        (DMA'd in place, no staging copy)."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "detect_batch")
        pb, k1 = make_params(params_bright)
        pd, k2 = make_params(params_dim, dim=True)
        c, k3 = self._catalog(cat)
        res = np.zeros(n, RESULT_DTYPE)
        self._chk(self._lib.lfdmi_detect_batch_raw(self._h, _ptr(frames), code, n, h, w,
                                                   C.byref(c) if c is not None else None,
                                                   C.byref(rs) if rs is not None else None,
                                                   C.byref(pb), C.byref(pd), _ptr(res), loc))
        return res

    # -- detection rounds (lfdmi_detect_rounds) --------------------------------------------------------------------------------
    def detect_rounds(self, frames, params_bright, params_dim, cat=None, rs=None, pinned=False, **params):
        """Up to ``max_trails`` trails per frame (include/lfdmi.h: detection rounds): ``detect_batch``, then the band of every
        line found so far blotted on a work copy of the frames that found one, and ``detect_batch`` again.  frames, cat, rs,
        pinned: as ``detect_batch`` takes them, and the frames are left as it leaves them.  params: max_trails, half, dup_dist.
        Returns (RESULT_DTYPE records [n, max_trails], int32 n_found [n], int32 dup_of [n, max_trails])."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "detect_rounds")
        p = make_rounds_params(**params)
        pb, k1 = make_params(params_bright)
        pd, k2 = make_params(params_dim, dim=True)
        c, k3 = self._catalog(cat)
        K = max(1, int(p.max_trails))
        rec = np.zeros((n, K), RESULT_DTYPE)
        n_found = np.zeros(n, np.int32)
        dup_of = np.full((n, K), -1, np.int32)
        self._chk(self._lib.lfdmi_detect_rounds(self._h, _ptr(frames), code, n, h, w,
                                                C.byref(c) if c is not None else None,
                                                C.byref(rs) if rs is not None else None,
                                                C.byref(pb), C.byref(pd), C.byref(p), _ptr(rec), _ptr(n_found), _ptr(dup_of), loc))
        return rec, n_found, dup_of

    # -- calls in flight (lfdmi_detect_batch_begin / lfdmi_process_multiscale_begin / lfdmi_end_oldest) ---------------------------
    def calls_in_flight(self):
        return int(self._lib.lfdmi_calls_in_flight(self._h))

    def _end_oldest(self):
        pend = self._inflight.pop(0)
        rc = self._lib.lfdmi_end_oldest(self._h)
        pend._finish(NativeError(rc, self._lib.lfdmi_last_error(self._h).decode()) if rc else None)

    def _begin(self, fn, args, res, keep, squeeze=False):
        self._chk(fn(self._h, *args))
        pend = Pending(self, res, keep, squeeze)
        self._inflight.append(pend)
        return pend

    def detect_batch_begin(self, frames, params_bright, params_dim, cat=None, rs=None, pinned=False):
        """``detect_batch`` without waiting: returns a ``Pending`` whose ``result()`` is what ``detect_batch`` returns.  Frames
        are device-resident (torch CUDA tensor, ``DeviceFrames``) or, with ``pinned=True``, in ``PinnedBuffer`` memory; they and
        the catalogue must stay untouched until the call has ended (LFDMI_MAX_CALLS_IN_FLIGHT = 2 calls at a time)."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "detect_batch_begin", contiguous=True)
        pb, k1 = make_params(params_bright)
        pd, k2 = make_params(params_dim, dim=True)
        c, k3 = self._catalog(cat)
        res = np.zeros(n, RESULT_DTYPE)
        args = (_ptr(frames), code, n, h, w, C.byref(c) if c is not None else None, C.byref(rs) if rs is not None else None,
                C.byref(pb), C.byref(pd), _ptr(res), loc)
        return self._begin(self._lib.lfdmi_detect_batch_begin, args, res, [frames, pb, pd, c, rs, k1, k2, k3, cat, args])

    def process_multiscale_begin(self, img, params, rhos, dim=True, flip=False, after_bright=False):
        """``process_multiscale`` without waiting (device-resident images): a ``Pending`` whose ``result()`` is its array."""
        img, n, h, w, sq = self._batch(img)
        if not _is_dev(img):
            raise ValueError("process_multiscale_begin needs device-resident images")
        p, keep = make_params(params, dim=dim)
        rh = (C.c_double * len(rhos))(*[float(r) for r in rhos])
        res = np.zeros((len(rhos), n), RESULT_DTYPE)
        args = (_ptr(img), _dtype_code(img), n, h, w, int(flip), int(dim), int(after_bright), C.byref(p), len(rhos), rh, _ptr(res), DEVICE)
        return self._begin(self._lib.lfdmi_process_multiscale_begin, args, res, [img, p, keep, rh, args], squeeze=sq)

    # -- trail profiles (lfdmi_measure_trails) ----------------------------------------------------------------------------------
    def measure_trails(self, frames, records, cat=None, rs=None, pinned=False, native_device=False, **params):
        """Refined line, extent, cross-section profile, fwhm and depth of every frame whose detection record has found != 0
        (include/lfdmi.h: trail profiles).  frames: what ``detect_batch`` took ('<f4' or '>f4' numpy, torch CUDA float32,
        ``DeviceFrames``), only read; records: its result array -- records of the flipped frame, as ``detect_batch`` (and
        ``process_bright`` / ``_dim`` / ``_multiscale`` with flip=True) return them.  ``DeviceFrames`` hold big-endian data
        until ``detect_batch`` has swapped them in place: ``native_device=True`` after that call.  Returns (TRAIL_DTYPE array
        [n], float32 profiles [n, 2K+1]); frames without a measurement have NaN rows."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "measure_trails", native_device=native_device)
        rec = np.ascontiguousarray(records, RESULT_DTYPE).reshape(-1)
        if len(rec) != n:
            raise ValueError(f"{len(rec)} records for {n} frames")
        p = make_trail_params(**params)
        c, keep = self._catalog(cat)
        out = np.zeros(n, TRAIL_DTYPE)
        prof = np.empty((n, trail_bins(p)), np.float32)
        self._chk(self._lib.lfdmi_measure_trails(self._h, _ptr(frames), code, n, h, w, loc, _ptr(rec),
                                                 C.byref(c) if c is not None else None, C.byref(rs) if rs is not None else None,
                                                 C.byref(p), _ptr(out), _ptr(prof)))
        return out, prof

    # -- defocus fit (lfdmi_fit_defocus) ---------------------------------------------------------------------------------------
    def fit_defocus(self, bank, trails, profiles, seeing=None, chi2_by_height=False):
        """Best defocus model of every trail (include/lfdmi.h: defocus fit).  bank: a ``defocus.DefocusBank`` of this context;
        trails / profiles: what ``measure_trails`` returned (with the trail params the bank was built for); seeing: None or n
        FWHM values in arcsec (NaN: free).  Returns a DEFOCUS_DTYPE array [n], and with chi2_by_height=True also the float32
        [n, n_h + 1] chi2 per height (the last column: the focus model)."""
        if not bank._b or bank.ctx is not self:
            raise ValueError("fit_defocus needs an open bank of this context")
        tr = np.ascontiguousarray(trails, TRAIL_DTYPE).reshape(-1)
        n = len(tr)
        prof = np.ascontiguousarray(profiles, np.float32)
        if prof.shape != (n, bank.n_bins):
            raise ValueError(f"profiles of shape {prof.shape}, the bank needs ({n}, {bank.n_bins})")
        see = None
        if seeing is not None:
            see = np.ascontiguousarray(np.broadcast_to(np.asarray(seeing, np.float32), (n,)))
        out = np.zeros(n, DEFOCUS_DTYPE)
        cbh = np.empty((n, bank.n_h + 1), np.float32) if chi2_by_height else None
        self._chk(self._lib.lfdmi_fit_defocus(self._h, bank._b, _ptr(tr), _ptr(prof), n, _ptr(see), _ptr(out), _ptr(cbh)))
        return (out, cbh) if chi2_by_height else out

    # -- trail injection (lfdmi_inject_trails) ----------------------------------------------------------------------------------
    def inject_trails(self, frames, trails, tables, table_step, subsample=4, pinned=False):
        """Add model trails to ``frames`` in place (include/lfdmi.h: trail injection).  frames: float32 (n, h, w) or (h, w), a
        torch CUDA tensor (rendered where it is), ``NativeDeviceFrames`` or a C-contiguous numpy array (the frames that carry a
        trail are uploaded, rendered and copied back; ``pinned=True``: the array lives in ``PinnedBuffer`` memory); big-endian
        frames are refused.  trails: INJECT_DTYPE records (or anything ``np.asarray`` turns into them); tables: float32
        (n_tables, 2M+1) or one row, node k at (k - M) * table_step px from the line.  Returns ``frames``."""
        if not _is_dev(frames) and not (isinstance(frames, np.ndarray) and frames.flags.c_contiguous and frames.flags.writeable):
            raise ValueError("inject_trails needs a writable C-contiguous array (it is modified in place)")
        fr, code, n, h, w, loc = self._frames(frames, pinned, "inject_trails")
        tr = np.ascontiguousarray(trails, INJECT_DTYPE).reshape(-1)
        tab = np.ascontiguousarray(tables, np.float32)
        if tab.ndim == 1:
            tab = tab[None]
        if tab.ndim != 2:
            raise ValueError("tables: (n_tables, 2M+1) float32")
        self._chk(self._lib.lfdmi_inject_trails(self._h, _ptr(fr), code, n, h, w, loc, _ptr(tr), len(tr), _ptr(tab), tab.shape[0],
                                                tab.shape[1], C.c_double(float(table_step)), int(subsample)))
        return frames

    # -- trail masks (lfdmi_mask_trails) ------------------------------------------------------------------------------------------
    def mask_trails(self, frames, segments, shape=None, mask=None, fill="none", clear=True, pinned=False):
        """Flag, and optionally fill, the pixels of every segment's band (include/lfdmi.h: trail masks).  frames: float32 (n, h, w)
        or (h, w) as ``inject_trails`` takes them, filled in place (a torch CUDA tensor where it is); None with fill="none", when
        ``shape`` = (n, h, w) or (h, w) or the mask gives the size.  segments: MASK_SEGMENT_DTYPE records (or anything
        ``np.asarray`` turns into them), coordinates of the flipped frame.  mask: None (a new uint8 plane set, on the device when
        the frames are), False (fill only), or a uint8 array / torch CUDA tensor of the frames' shape, which stays where it is and
        is ORed onto unless ``clear``.  fill: "none", "zero", "nan" or "value".  ``pinned=True``: the host arrays live in
        ``PinnedBuffer`` memory.  Returns (mask or None, MASK_STAT_DTYPE records [n_seg], int32 counts per frame [n])."""
        p = make_mask_params(fill_mode=fill, clear=int(bool(clear)))
        fr, code, loc, sq = None, F32, HOST, False
        if frames is not None:
            if p.fill_mode != MASK_FILL_NONE and not _is_dev(frames) and not (
                    isinstance(frames, np.ndarray) and frames.flags.c_contiguous and frames.flags.writeable):
                raise ValueError("mask_trails fills a writable C-contiguous array (it is modified in place)")
            fr, code, n, h, w, loc = self._frames(frames, pinned, "mask_trails")
            sq = len(tuple(fr.shape)) == 2
        elif shape is not None:
            shp = tuple(int(v) for v in shape)
            sq = len(shp) == 2
            n, h, w = (1, *shp) if sq else shp
        elif mask is not None and mask is not False:
            shp = tuple(mask.shape)
            sq = len(shp) == 2
            n, h, w = (1, *shp) if sq else shp
        else:
            raise ValueError("mask_trails needs frames, a shape or a mask")
        own = mask is None                                 # (an array made here is pageable, whatever ``pinned`` says of the caller's)
        if mask is None:
            if _is_dev(fr):
                import torch
                mask = torch.empty((h, w) if sq else (n, h, w), dtype=torch.uint8, device=fr.device)   # (the library clears it)
            else:
                mask = np.zeros((h, w) if sq else (n, h, w), np.uint8)
            p.clear = 1
        elif mask is False:
            mask = None
        else:
            if tuple(mask.shape) not in ((n, h, w), (h, w) if n == 1 else None):
                raise ValueError(f"mask of shape {tuple(mask.shape)} for frames of shape {(n, h, w)}")
            if str(mask.dtype).replace("torch.", "") != "uint8":
                raise TypeError("mask_trails needs a uint8 mask")
            if _is_dev(mask):
                if not mask.is_contiguous():
                    raise ValueError("device tensors must be contiguous")
            elif not (isinstance(mask, np.ndarray) and mask.flags.c_contiguous and mask.flags.writeable):
                raise ValueError("mask_trails needs a writable C-contiguous mask (it is written in place)")
        mloc = DEVICE if _is_dev(mask) else (HOST_PINNED if pinned and not own else HOST)
        sg = np.ascontiguousarray(segments, MASK_SEGMENT_DTYPE).reshape(-1)
        stats = np.zeros(len(sg), MASK_STAT_DTYPE)
        counts = np.zeros(n, np.int32)
        self._chk(self._lib.lfdmi_mask_trails(self._h, _ptr(fr), code, n, h, w, loc, _ptr(sg), len(sg), C.byref(p), _ptr(mask), mloc,
                                              _ptr(stats), _ptr(counts)))
        return mask, stats, counts

    # -- light curves (lfdmi_light_curves) ----------------------------------------------------------------------------------------
    def light_curves(self, frames, segs, mask=None, skip_bits=0, sigma=None, max_sections=256, pinned=False, native_device=False,
                     **params):
        """The brightness along every segment in sections (include/lfdmi.h: light curves).  frames: what ``stack_profiles`` takes
        ('<f4' or '>f4' numpy, torch CUDA float32, ``DeviceFrames``), only read; segs: LC_SEGMENT_DTYPE records (or anything
        ``np.asarray`` turns into them), coordinates of the flipped frame; mask: None or the uint8 planes of ``mask_trails`` where
        the frames are (numpy with host frames, a torch CUDA tensor with device frames), a pixel with ``mask & skip_bits`` is
        left out; sigma: None (0.025), a number or n values; params: fields of lfdmi_lc_params.  Returns (LC_DTYPE records
        [n_seg], LC_SECTION_DTYPE records [n_seg, max_sections])."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "light_curves", native_device=native_device)
        sg = np.ascontiguousarray(segs, LC_SEGMENT_DTYPE).reshape(-1)
        p = make_lc_params(**params)
        sig = _sigma(sigma, n)
        m = int(max_sections)
        if not 1 <= m <= LC_MAX_SECTIONS:
            raise ValueError(f"max_sections: 1 .. {LC_MAX_SECTIONS}")
        if mask is not None:
            shp = tuple(mask.shape)
            if shp != (n, h, w) and not (n == 1 and shp == (h, w)):      # (one frame may come with a 2-d plane)
                raise ValueError(f"mask of shape {shp} for frames of shape {(n, h, w)}")
            if str(mask.dtype).replace("torch.", "") != "uint8":
                raise TypeError("light_curves needs a uint8 mask")
            if _is_dev(mask) != (loc == DEVICE):
                raise ValueError("light_curves needs the mask where the frames are")
            if _is_dev(mask):
                if not mask.is_contiguous():
                    raise ValueError("device tensors must be contiguous")
            else:
                mask = np.ascontiguousarray(mask)
        out = np.zeros(len(sg), LC_DTYPE)
        sec = np.zeros((len(sg), m), LC_SECTION_DTYPE)
        self._chk(self._lib.lfdmi_light_curves(self._h, _ptr(frames), code, n, h, w, loc, _ptr(mask), int(skip_bits), _ptr(sg), len(sg),
                                               _ptr(sig), C.byref(p), _ptr(out), _ptr(sec), m))
        return out, sec

    # -- trail strips (lfdmi_trail_strips) ----------------------------------------------------------------------------------------
    def trail_strips(self, frames, segs, mask=None, skip_bits=0, sigma=None, max_sections=256, max_cells=None, pinned=False,
                     native_device=False, **params):
        """The straightened band of every segment (include/lfdmi.h: trail strips).  frames, segs' coordinates, mask, skip_bits and
        sigma: what ``light_curves`` takes; segs: STRIP_SEGMENT_DTYPE records; params: fields of lfdmi_strip_params.  max_cells:
        the cells a segment may have (default: what the longest segment of the call needs, at most max_sections x 129).  Returns
        (STRIP_DTYPE records [n_seg], STRIP_SECTION_DTYPE records [n_seg, max_sections], STRIP_CELL_DTYPE records [n_seg,
        max_cells]); cell (j, b) of segment i is [i, j * n_off + b]."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "trail_strips", native_device=native_device)
        sg = np.ascontiguousarray(segs, STRIP_SEGMENT_DTYPE).reshape(-1)
        p = make_strip_params(**params)
        sig = _sigma(sigma, n)
        m = int(max_sections)
        if not 1 <= m <= STRIP_MAX_SECTIONS:
            raise ValueError(f"max_sections: 1 .. {STRIP_MAX_SECTIONS}")
        if max_cells is None:
            max_cells = strip_cells_needed(sg, p, m)
        mc = int(max_cells)
        if not 1 <= mc <= STRIP_MAX_SECTIONS * STRIP_MAX_OFF:
            raise ValueError(f"max_cells: 1 .. {STRIP_MAX_SECTIONS * STRIP_MAX_OFF}")
        if mask is not None:
            shp = tuple(mask.shape)
            if shp != (n, h, w) and not (n == 1 and shp == (h, w)):      # (one frame may come with a 2-d plane)
                raise ValueError(f"mask of shape {shp} for frames of shape {(n, h, w)}")
            if str(mask.dtype).replace("torch.", "") != "uint8":
                raise TypeError("trail_strips needs a uint8 mask")
            if _is_dev(mask) != (loc == DEVICE):
                raise ValueError("trail_strips needs the mask where the frames are")
            if _is_dev(mask):
                if not mask.is_contiguous():
                    raise ValueError("device tensors must be contiguous")
            else:
                mask = np.ascontiguousarray(mask)
        out = np.zeros(len(sg), STRIP_DTYPE)
        sec = np.zeros((len(sg), m), STRIP_SECTION_DTYPE)
        cells = np.zeros((len(sg), mc), STRIP_CELL_DTYPE)
        self._chk(self._lib.lfdmi_trail_strips(self._h, _ptr(frames), code, n, h, w, loc, _ptr(mask), int(skip_bits), _ptr(sg), len(sg),
                                               _ptr(sig), C.byref(p), _ptr(out), _ptr(sec), m, _ptr(cells), mc))
        return out, sec, cells

    # -- trail subtraction (lfdmi_subtract_trails) --------------------------------------------------------------------------------
    def subtract_trails(self, frames, segs, mask=None, skip_bits=0, max_sections=256, max_cells=None, want_model=False, pinned=False,
                        native_device=False, **params):
        """Model every segment's trail from its own strip and subtract it from ``frames`` in place (include/lfdmi.h: trail
        subtraction).  frames: as ``inject_trails`` takes them (a torch CUDA tensor is changed where it is; of a numpy array the
        frames that carry a good segment are uploaded, changed and copied back); with ``apply=0`` nothing is written and what
        ``trail_strips`` takes is accepted, big-endian frames too.  segs: STRIP_SEGMENT_DTYPE records; mask, skip_bits,
        max_sections, max_cells: as ``trail_strips``; params: fields of lfdmi_sub_params.  Returns (SUB_DTYPE records [n_seg],
        and with ``want_model`` the float32 tables [n_seg, max_cells], cell (j, b) of segment i at [i, j * n_off + b], else None)."""
        p = make_sub_params(**params)
        if p.apply and not isinstance(frames, DeviceFrames) and not _is_dev(frames) and not (
                isinstance(frames, np.ndarray) and frames.flags.c_contiguous and frames.flags.writeable):
            raise ValueError("subtract_trails needs a writable C-contiguous array (it is modified in place)")
        frames, code, n, h, w, loc = self._frames(frames, pinned, "subtract_trails", native_device=native_device)
        sg = np.ascontiguousarray(segs, STRIP_SEGMENT_DTYPE).reshape(-1)
        m = int(max_sections)
        if not 1 <= m <= STRIP_MAX_SECTIONS:
            raise ValueError(f"max_sections: 1 .. {STRIP_MAX_SECTIONS}")
        if max_cells is None:
            max_cells = strip_cells_needed(sg, p, m)
        mc = int(max_cells)
        if not 1 <= mc <= STRIP_MAX_SECTIONS * STRIP_MAX_OFF:
            raise ValueError(f"max_cells: 1 .. {STRIP_MAX_SECTIONS * STRIP_MAX_OFF}")
        if mask is not None:
            shp = tuple(mask.shape)
            if shp != (n, h, w) and not (n == 1 and shp == (h, w)):      # (one frame may come with a 2-d plane)
                raise ValueError(f"mask of shape {shp} for frames of shape {(n, h, w)}")
            if str(mask.dtype).replace("torch.", "") != "uint8":
                raise TypeError("subtract_trails needs a uint8 mask")
            if _is_dev(mask) != (loc == DEVICE):
                raise ValueError("subtract_trails needs the mask where the frames are")
            if _is_dev(mask):
                if not mask.is_contiguous():
                    raise ValueError("device tensors must be contiguous")
            else:
                mask = np.ascontiguousarray(mask)
        out = np.zeros(len(sg), SUB_DTYPE)
        model = np.zeros((len(sg), mc), np.float32) if want_model else None
        self._chk(self._lib.lfdmi_subtract_trails(self._h, _ptr(frames), code, n, h, w, loc, _ptr(mask), int(skip_bits), _ptr(sg), len(sg),
                                                  None, C.byref(p), _ptr(out), _ptr(model), m, mc))
        return out, model

    # -- stacked cross-sections (lfdmi_stack_profiles) ----------------------------------------------------------------------------
    def stack_profiles(self, frames, segments, sigma=None, pinned=False, native_device=False, raw=False, **params):
        """The stacked cross-section of every segment (include/lfdmi.h: stacked cross-sections).  frames: what ``Radon.search``
        takes ('<f4' or '>f4' numpy, torch CUDA float32, ``DeviceFrames``), only read; segments: STACK_SEGMENT_DTYPE records (or
        anything ``np.asarray`` turns into them), coordinates of the flipped frame; sigma: None (0.025), a number or n values.
        Returns (STACK_DTYPE records [n_seg], float32 rows [n_seg, 2K+1]); with raw=True also the last pass's sums (float32
        [n_seg, 2, 2K+1]: left and right half) and counts (int32, the same shape)."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "stack_profiles", native_device=native_device)
        sg = np.ascontiguousarray(segments, STACK_SEGMENT_DTYPE).reshape(-1)
        p = make_stack_params(**params)
        sig = _sigma(sigma, n)
        nb = max(1, stack_bins(p)) if p.step > 0 and np.isfinite(p.prof_half / p.step) and p.prof_half / p.step < 1e6 else 1
        out = np.zeros(len(sg), STACK_DTYPE)
        prof = np.empty((len(sg), nb), np.float32)
        sums = np.zeros((len(sg), 2, nb), np.float32) if raw else None
        cnts = np.zeros((len(sg), 2, nb), np.int32) if raw else None
        self._chk(self._lib.lfdmi_stack_profiles(self._h, _ptr(frames), code, n, h, w, loc, _ptr(sg), len(sg), _ptr(sig), C.byref(p),
                                                 _ptr(out), _ptr(prof), _ptr(sums), _ptr(cnts)))
        return (out, prof, sums, cnts) if raw else (out, prof)

    # -- source finder (lfdmi_find_stars / lfdmi_stars_catalog) ---------------------------------------------------------------------
    def find_stars(self, frames, sigma=None, pinned=False, native_device=False, device_out=False, **params):
        """The compact sources of every frame (include/lfdmi.h: source finder).  frames: what ``stack_profiles`` takes, only read;
        sigma: None (0.025), a number or one value per frame.  Returns (STAR_DTYPE records [n, max_obj], STARS_FRAME_DTYPE records
        [n]); with device_out=True the records stay on the device (a torch uint8 tensor [n, max_obj, 32]) for ``stars_catalog``."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "find_stars", native_device=native_device)
        p = make_stars_params(**params)
        sig = _sigma(sigma, n)
        frec = np.zeros(n, STARS_FRAME_DTYPE)
        m = max(1, min(int(p.max_obj), STARS_MAX_OBJ))
        if device_out:
            import torch
            rec = torch.empty((n, m, STAR_DTYPE.itemsize), dtype=torch.uint8, device=f"cuda:{self.device}")   # (the library writes every byte)
        else:
            rec = np.zeros((n, m), STAR_DTYPE)
        self._chk(self._lib.lfdmi_find_stars(self._h, _ptr(frames), code, n, h, w, loc, _ptr(sig), C.byref(p), _ptr(rec),
                                             DEVICE if device_out else HOST, _ptr(frec)))
        return rec, frec

    def stars_catalog(self, records, frame_records, pixscale=0.396, device=False):
        """Step 8 of the source finder: the catalogue dict ``synth.pack_catalogs`` returns (count, ROWC, COLC, PSFMAG, PETROTH90,
        NOBSERVE, NDETECT), filled on the device from the records of ``find_stars`` (numpy, or its device tensor); device=True:
        torch CUDA arrays, which ``detect_batch`` and ``remove_stars`` take in place."""
        frec = np.ascontiguousarray(frame_records, STARS_FRAME_DTYPE).reshape(-1)
        n = len(frec)
        if _is_dev(records):
            m = int(records.shape[1])
        else:
            records = np.ascontiguousarray(records, STAR_DTYPE).reshape(n, -1)
            m = records.shape[1]
        if device:
            import torch
            dev = f"cuda:{self.device}"
            # (torch.empty: the library writes every row and count on its own stream; a fill kernel on torch's stream would race it)
            cat = {"count": torch.empty(n, dtype=torch.int32, device=dev)}
            for k in CATALOG_KEYS5:
                cat[k] = torch.empty((n, m, 5), dtype=torch.float32, device=dev)
            for k in ("NOBSERVE", "NDETECT"):
                cat[k] = torch.empty((n, m), dtype=torch.int32, device=dev)
        else:
            cat = {"count": np.zeros(n, np.int32)}
            for k in CATALOG_KEYS5:
                cat[k] = np.zeros((n, m, 5), np.float32)
            for k in ("NOBSERVE", "NDETECT"):
                cat[k] = np.zeros((n, m), np.int32)
        c, keep = self._catalog(cat)
        self._chk(self._lib.lfdmi_stars_catalog(self._h, _ptr(records), DEVICE if _is_dev(records) else HOST, _ptr(frec), n, m,
                                                float(pixscale), C.byref(c)))
        return cat

    # -- frame seeing (lfdmi_measure_seeing) ---------------------------------------------------------------------------------------
    def measure_seeing(self, frames, records, frame_records, sigma=None, pinned=False, native_device=False, **params):
        """The second moments of every frame's good stars and the frame's PSF width (include/lfdmi.h: frame seeing).  frames,
        sigma: what ``find_stars`` took; records, frame_records: what it returned (numpy, or its device tensor with
        device_out=True).  Returns (PSF_STAR_DTYPE records [n, max_used], SEEING_FRAME_DTYPE records [n])."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "measure_seeing", native_device=native_device)
        p = make_psf_params(**params)
        sig = _sigma(sigma, n)
        frec = np.ascontiguousarray(frame_records, STARS_FRAME_DTYPE).reshape(-1)
        if len(frec) != n:
            raise ValueError("measure_seeing: one frame record per frame")
        if _is_dev(records):
            if int(records.shape[0]) != n:
                raise ValueError("measure_seeing: records of another number of frames")
            m = int(records.shape[1])
        else:
            records = np.ascontiguousarray(records, STAR_DTYPE)
            records = records.reshape(n, -1) if n else records.reshape(0, 1)
            m = records.shape[1]
        mu = max(1, min(int(p.max_used), PSF_MAX_USED))
        out = np.zeros((n, mu), PSF_STAR_DTYPE)
        ofr = np.zeros(n, SEEING_FRAME_DTYPE)
        self._chk(self._lib.lfdmi_measure_seeing(self._h, _ptr(frames), code, n, h, w, loc, _ptr(sig), _ptr(records),
                                                 DEVICE if _is_dev(records) else HOST, _ptr(frec), m, C.byref(p), _ptr(out), _ptr(ofr)))
        return out, ofr

    # -- frame previews (lfdmi_frame_previews) --------------------------------------------------------------------------------------
    def frame_previews(self, frames, lut=None, limits=None, pinned=False, native_device=False, out_device=False, want_cells=False,
                       **params):
        """Binned, stretched 8-bit images of the flipped frames (include/lfdmi.h: frame previews).  frames: what ``find_stars``
        takes, only read.  params: bin, mode ("rank" / "given"), lo_ppm, hi_ppm.  limits: with mode="given", (lo, hi) or one pair
        per frame, in the frames' units.  lut: 4096 bytes (default: ``previews.lut()``).  Returns (uint8 images [n, Hp, Wp],
        PREVIEW_FRAME_DTYPE records [n]), with want_cells=True (images, int64 cell means [n, Hp, Wp], records); out_device=True:
        images and cells stay on the device as torch tensors."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "frame_previews", native_device=native_device)
        p = make_preview_params(**params)
        if lut is None:
            from .previews import lut as default_lut
            lut = default_lut()
        lut = np.ascontiguousarray(lut, np.uint8).reshape(-1)
        if lut.size != PREVIEW_LUT:
            raise ValueError(f"frame_previews: lut holds {PREVIEW_LUT} bytes")
        lim = None
        if limits is not None:
            lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limits, np.float64), (n, 2)))
        elif p.mode == PREVIEW_GIVEN:
            raise ValueError("frame_previews: mode='given' needs limits")
        b = int(p.bin) if int(p.bin) in PREVIEW_BINS else 1     # (a bad bin: the library refuses it; the arrays just have to exist)
        shape = (n, -(-h // b), -(-w // b))
        cells = None
        if out_device:
            import torch
            dev = f"cuda:{self.device}"
            out = torch.empty(shape, dtype=torch.uint8, device=dev)        # (the library writes every byte on its own stream)
            if want_cells:
                cells = torch.empty(shape, dtype=torch.int64, device=dev)
        else:
            out = np.zeros(shape, np.uint8)
            if want_cells:
                cells = np.zeros(shape, np.int64)
        rec = np.zeros(n, PREVIEW_FRAME_DTYPE)
        self._chk(self._lib.lfdmi_frame_previews(self._h, _ptr(frames), code, n, h, w, loc, C.byref(p), _ptr(lim), _ptr(lut), _ptr(out),
                                                 DEVICE if out_device else HOST, _ptr(cells), _ptr(rec)))
        return (out, cells, rec) if want_cells else (out, rec)

    # -- short-streak search (lfdmi_streak_search) -----------------------------------------------------------------------------------
    def streak_search(self, frames, sigma=None, pinned=False, native_device=False, **params):
        """The short streaks of every frame (include/lfdmi.h: short-streak search).  frames: what ``find_stars`` takes, only read;
        sigma: None (0.025), a number or one value per frame; ``params``: the fields of lfdmi_streak_params.  Returns
        (STREAK_DTYPE records [n, max_streaks], int32 n_streaks [n])."""
        frames, code, n, h, w, loc = self._frames(frames, pinned, "streak_search", native_device=native_device)
        p = make_streak_params(**params)
        sig = _sigma(sigma, n)
        m = max(1, min(int(p.max_streaks), STREAK_MAX_STREAKS))
        rec = np.zeros((n, m), STREAK_DTYPE)
        ns = np.zeros(n, np.int32)
        self._chk(self._lib.lfdmi_streak_search(self._h, _ptr(frames), code, n, h, w, loc, _ptr(sig), C.byref(p), _ptr(rec), _ptr(ns)))
        return rec, ns

    def pinned_buffer(self, nbytes):
        """Page-locked host memory next to this context's GPU (lfdmi_host_alloc) as a ``PinnedBuffer``."""
        return PinnedBuffer(self, nbytes)

    def get_counters(self, slot0=0, n=None):
        """Work counters ([n, 22] int32, see LFDMI_COUNTERS) the last pass left for in-flight slots slot0 .. slot0+n-1."""
        n = self.max_inflight - slot0 if n is None else int(n)
        out = np.zeros((n, 22), np.int32)
        self._chk(self._lib.lfdmi_get_counters(self._h, int(slot0), n, _ptr(out)))
        return out

    def get_stage(self, slot, which, h, w):
        out = np.empty((h, w), np.uint8)
        self._chk(self._lib.lfdmi_get_stage(self._h, int(slot), int(which), int(h), int(w), _ptr(out), HOST))
        return out


class _Handle:
    """What ``Sky`` and ``Radon`` share: a library handle made on a context for frames of one shape, closed with the context
    at the latest.  A subclass names itself (``_what``), its params function, its create and destroy symbols and the attribute
    its handle is read under (``_attr``)."""

    def __init__(self, ctx, shape, max_frames=None, **params):
        setattr(self, self._attr, C.c_void_p())
        self._lib = lib()
        self.ctx = ctx
        if not getattr(ctx, "_h", None):
            raise ValueError("the context is closed")
        self.shape = (int(shape[0]), int(shape[1]))
        self.max_frames = int(ctx.max_inflight if max_frames is None else max_frames)
        self.params = self._make_params(**params)
        ctx._chk(getattr(self._lib, self._create)(ctx._h, self.shape[0], self.shape[1], self.max_frames, C.byref(self.params),
                                                   C.byref(getattr(self, self._attr))))
        import weakref
        ctx.__dict__.setdefault("_skies", weakref.WeakSet()).add(self)

    def close(self):
        if getattr(self, self._attr, None):
            getattr(self._lib, self._destroy)(getattr(self, self._attr))
            setattr(self, self._attr, C.c_void_p())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self, need_ctx=True):
        """the handle, refused when it (or, for a call, its context) is closed"""
        if not getattr(self, self._attr) or (need_ctx and not getattr(self.ctx, "_h", None)):
            raise ValueError(f"the {self._what} handle is closed")
        return getattr(self, self._attr)

    def _frames(self, frames, pinned, what, **kw):
        """``Context._frames`` of frames that must have the handle's shape"""
        frames, code, n, h, w, loc = self.ctx._frames(frames, pinned, what, **kw)
        if (h, w) != self.shape:
            raise NativeError(ERR_ARG, f"{what}: frames of {h} x {w}, the handle was made for {self.shape[0]} x {self.shape[1]}")
        return frames, code, n, h, w, loc


class Sky(_Handle):
    """lfdmi_sky: the sky normalisation of frames of ``shape`` on ``ctx``'s device (include/lfdmi.h: sky normalisation).  The
    handle owns the meshes and a device buffer of ``max_frames`` normalised frames; ``Context.close()`` closes it first."""
    _what, _attr, _create, _destroy = "sky", "_s", "lfdmi_sky_create", "lfdmi_sky_destroy"
    _make_params = staticmethod(make_sky_params)

    def __init__(self, ctx, shape, max_frames=None, **params):
        super().__init__(ctx, shape, max_frames, **params)
        ny, nx, nb = C.c_int32(), C.c_int32(), C.c_int64()
        self._lib.lfdmi_sky_dims(self._s, C.byref(ny), C.byref(nx), C.byref(nb))
        self.ny, self.nx, self.bytes = ny.value, nx.value, nb.value

    def frames(self, n=None):
        """The handle's device buffer as ``DeviceFrames`` (``NativeDeviceFrames``: native float32)."""
        n = self.max_frames if n is None else int(n)
        return NativeDeviceFrames(self._lib.lfdmi_sky_frames(self._open(need_ctx=False)), (n, *self.shape))

    def normalize(self, frames, out=None, meshes=False, pinned=False):
        """Normalise ``frames`` ('<f4' / '>f4' numpy, torch CUDA float32, ``DeviceFrames`` holding big-endian data).  out: None =
        the handle's device buffer (``frames(n)``; n <= max_frames), "inplace" for torch CUDA float32 frames, or a float32 numpy
        array / torch CUDA tensor of the frames' shape.  Returns the SKY_DTYPE records [n], and with meshes=True also the
        filtered sky and sigma meshes, float32 [n, ny, nx] each."""
        s, ctx = self._open(), self.ctx
        frames, code, n, h, w, loc = self._frames(frames, pinned, "Sky.normalize")
        if isinstance(out, str):
            if out != "inplace":
                raise ValueError("out: None, 'inplace' or an array")
            out = frames
        out_loc = HOST
        if out is not None:
            if not _is_dev(out) and not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous):
                raise TypeError("out: a C-contiguous float32 numpy array or a torch CUDA tensor")
            if int(np.prod(tuple(out.shape))) != n * h * w:
                raise ValueError("out does not have the frames' size")
            out_loc = DEVICE if _is_dev(out) else HOST
        rec = np.zeros(n, SKY_DTYPE)
        mb = np.empty((n, self.ny, self.nx), np.float32) if meshes else None
        ms = np.empty((n, self.ny, self.nx), np.float32) if meshes else None
        ctx._chk(self._lib.lfdmi_sky_normalize(ctx._h, s, _ptr(frames), code, n, loc, _ptr(out), out_loc, _ptr(rec), _ptr(mb),
                                               _ptr(ms)))
        return (rec, mb, ms) if meshes else rec


class Radon(_Handle):
    """lfdmi_radon: the faint-trail search of frames of ``shape`` on ``ctx``'s device (include/lfdmi.h: faint-trail search).
    The handle owns the transform's planes for ``max_frames`` frames; ``Context.close()`` closes it first."""
    _what, _attr, _create, _destroy = "radon", "_r", "lfdmi_radon_create", "lfdmi_radon_destroy"
    _make_params = staticmethod(make_radon_params)

    def __init__(self, ctx, shape, max_frames=None, **params):
        super().__init__(ctx, shape, max_frames, **params)
        self.p01, self.p23, self.bytes = self.dims()

    def dims(self):
        """(P of orientations 0 and 1, P of orientations 2 and 3, device bytes held)"""
        a, b, nb = C.c_int32(), C.c_int32(), C.c_int64()
        self.ctx._chk(self._lib.lfdmi_radon_dims(self._r, C.byref(a), C.byref(b), C.byref(nb)))
        return a.value, b.value, nb.value

    def search(self, frames, sigma=None, pinned=False, native_device=False):
        """The line of largest signal-to-noise of every frame ('<f4' / '>f4' numpy, torch CUDA float32, ``DeviceFrames``), only
        read.  sigma: None (0.025), a number or n values, the frames' sky sigma.  Returns RADON_DTYPE records [n]."""
        r, ctx = self._open(), self.ctx
        frames, code, n, h, w, loc = self._frames(frames, pinned, "Radon.search", native_device=native_device)
        sg = _sigma(sigma, n)
        res = np.zeros(n, RADON_DTYPE)
        ctx._chk(self._lib.lfdmi_radon_search(ctx._h, r, _ptr(frames), code, n, loc, _ptr(sg), _ptr(res)))
        return res

    def _peel(self, what, make, params, dtype, plain, frames, sigma, pinned, native_device):
        """the peeling search lfdmi_radon_<what>: ``make(**params)`` its params struct, ``dtype`` its records'; plain: None
        where the call has no such argument"""
        r, ctx = self._open(), self.ctx
        p = make(**params)
        frames, code, n, h, w, loc = self._frames(frames, pinned, "Radon." + what, native_device=native_device)
        sg = _sigma(sigma, n)
        k = max(1, min(int(p.max_lines), RADON_MAX_LINES))      # (out of range: the library refuses before it writes)
        res = np.zeros((n, k), dtype)
        nl = np.zeros(n, np.int32)
        pl = np.zeros(n, RADON_DTYPE) if plain else None
        ctx._chk(getattr(self._lib, "lfdmi_radon_" + what)(ctx._h, r, _ptr(frames), code, n, loc, _ptr(sg), C.byref(p), _ptr(res),
                                                            _ptr(nl), *(() if plain is None else (_ptr(pl),))))
        return (res, nl, pl) if plain else (res, nl)

    def search_lines(self, frames, sigma=None, max_lines=4, peel_halfwidth=8, min_seg=64, pinned=False, native_device=False):
        """Up to ``max_lines`` lines per frame by peeling, each with its extent (include/lfdmi.h: faint-trail search, steps
        7 - 9); frames and sigma as in ``search``.  Returns (RADON_LINE_DTYPE records [n, max_lines], n_lines [n]): a frame's
        found lines are its records 0 .. n_lines-1 in peel order, record n_lines (if there is room) is the round that stopped
        it.  The first call allocates the second V, M set; ``dims()`` counts it from then on."""
        return self._peel("search_lines", make_radon_lines_params, {"max_lines": max_lines, "peel_halfwidth": peel_halfwidth,
                                                                    "min_seg": min_seg},
                          RADON_LINE_DTYPE, None, frames, sigma, pinned, native_device)

    def search_short(self, frames, sigma=None, plain=False, pinned=False, native_device=False, **params):
        """Short trails: every stored level of the transform scored strip by strip, the best candidate's parent line, its
        extent, and peeling rounds as in ``search_lines`` (include/lfdmi.h: faint-trail search, steps 10 - 12); frames and
        sigma as in ``search``, ``params`` the fields of lfdmi_radon_short_params.  Returns (RADON_SHORT_DTYPE records
        [n, max_lines], n_lines [n]) and, with ``plain``, a third item: the RADON_DTYPE records ``search`` returns for these
        frames.  The first call allocates the rounds' buffers and the partial records; ``dims()`` counts them from then on."""
        return self._peel("search_short", make_radon_short_params, params, RADON_SHORT_DTYPE, bool(plain), frames, sigma, pinned,
                          native_device)

    def search_wide(self, frames, sigma=None, plain=False, pinned=False, native_device=False, **params):
        """Wide trails: bands of 1, 2, 4, .. ``max_width`` neighbouring lines of the last level scored as one, the best band's
        centre line, width and extent, and peeling rounds as in ``search_lines`` (include/lfdmi.h: faint-trail search, steps
        13 - 16); frames and sigma as in ``search``, ``params`` the fields of lfdmi_radon_wide_params.  Returns
        (RADON_WIDE_DTYPE records [n, max_lines], n_lines [n]) and, with ``plain``, a third item: the RADON_DTYPE records
        ``search`` returns for these frames.  The first call allocates the rounds' buffers and the partial records;
        ``dims()`` counts them from then on."""
        return self._peel("search_wide", make_radon_wide_params, params, RADON_WIDE_DTYPE, bool(plain), frames, sigma, pinned,
                          native_device)

    def null(self, frames, K=16, kind="lines", sigma=None, seeds=None, pinned=False, native_device=False, scheme="scramble", peel=None,
             **kind_params):
        """The null peaks of every frame: record 0 of the ``kind`` search ("lines", "short" or "wide") of K null realisations
        of each frame (include/lfdmi.h: faint-trail search, null peaks, steps 17 - 22); frames and sigma as in ``search``.
        seeds: None (frame f has seed f) or n uint64.  ``kind_params``: the fields of lfdmi_radon_short_params /
        lfdmi_radon_wide_params; "lines" takes none, but with another ``scheme`` or with ``peel`` those of
        lfdmi_radon_lines_params.  scheme: "scramble" (every pixel drawn from the frame), "signflip" (every pixel in its place,
        its sign by a coin), "rowshift" / "colshift" (every row / column rotated by its own offset).  peel ("signflip" only):
        RADON_PEEL_DTYPE records [n, n_peel], the lines of each frame whose bands are blotted before the search (width 0: none
        in this place).  Returns records [n, K]: RADON_DTYPE, RADON_SHORT_DTYPE or RADON_WIDE_DTYPE.  The first call of a kind
        allocates what that kind's search does; ``dims()`` counts it.  The defaults run lfdmi_radon_null, anything else
        lfdmi_radon_null_scheme."""
        r, ctx = self._open(), self.ctx
        if kind not in RADON_NULL_KINDS:
            raise ValueError("kind: 'lines', 'short' or 'wide'")
        if scheme not in RADON_NULL_SCHEMES:
            raise ValueError("scheme: 'scramble', 'signflip', 'rowshift' or 'colshift'")
        old = scheme == "scramble" and peel is None
        if kind == "lines" and kind_params and old:
            raise TypeError(f"unknown radon null parameter {sorted(kind_params)[0]!r}: kind 'lines' takes none")
        make = {"lines": make_radon_lines_params if kind_params else lambda: None, "short": make_radon_short_params,
                "wide": make_radon_wide_params}[kind]
        p = make(**kind_params)
        dtype = {"lines": RADON_DTYPE, "short": RADON_SHORT_DTYPE, "wide": RADON_WIDE_DTYPE}[kind]
        frames, code, n, h, w, loc = self._frames(frames, pinned, "Radon.null", native_device=native_device)
        sg = _sigma(sigma, n)
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, np.uint64).reshape(-1)
            if seeds.size != n:
                raise ValueError("seeds: one uint64 per frame")
        K = int(K)
        res = np.zeros((n, max(1, min(K, RADON_NULL_MAX))), dtype)       # (out of range: the library refuses before it writes)
        if old:
            ctx._chk(self._lib.lfdmi_radon_null(ctx._h, r, _ptr(frames), code, n, loc, _ptr(sg), _ptr(seeds), K, RADON_NULL_KINDS[kind],
                                                None if p is None else C.byref(p), _ptr(res)))
            return res
        n_peel = 0
        if peel is not None:
            peel = np.ascontiguousarray(peel, RADON_PEEL_DTYPE)
            if peel.ndim != 2 or peel.shape[0] != n:
                raise ValueError("peel: RADON_PEEL_DTYPE records [n, n_peel]")
            n_peel = peel.shape[1]
        ctx._chk(self._lib.lfdmi_radon_null_scheme(ctx._h, r, _ptr(frames), code, n, loc, _ptr(sg), _ptr(seeds), K, RADON_NULL_KINDS[kind],
                                                   None if p is None else C.byref(p), RADON_NULL_SCHEMES[scheme],
                                                   _ptr(peel) if n_peel else None, n_peel, _ptr(res)))
        return res
