"""SDSS-facing driver: which frames to process, in what order, and what gets written.

Host-side mirror of ``lfd/detecttrails/detecttrails.py``.  ``DetectTrails(**kwargs).process()``
keeps the reference's keyword interface, its three parameter dictionaries
(``params_bright`` / ``params_dim`` / ``params_removestars``, same keys and defaults,
detecttrails.py:202-239) and its frame-selection rules (detecttrails.py:290-342); per frame,
``process_field`` runs remove_stars -> vertical flip -> bright pass -> dim pass on the GPU
through one ``lfdmi_detect_batch`` call and appends a results row / an errors entry in the
reference's text formats.

Deliberate fixes of reference bugs: C8 ``params_dim=`` /
``params_removestars=`` keyword arguments land in their own dictionaries; C9 the results row
carries the 13 header values instead of literal ``{h['CRPIX2']}`` text.
"""
import bz2
import contextlib
import os
import traceback

import numpy as _np

from .. import _native
from . import fitslite, sdssfiles
from .loader import card_value, header_end, header_values
from .processfield import get_context, use_context, setup_debug, check_theta, dictify_hough  # noqa: F401
from .removestars import read_photoObj_arrays

# values of the cv2 constants the reference re-exports (detecttrails.py:14-18)
RETR_EXTERNAL, RETR_LIST, RETR_CCOMP, RETR_TREE = 0, 1, 2, 3
CHAIN_APPROX_NONE, CHAIN_APPROX_SIMPLE, CHAIN_APPROX_TC89_L1, CHAIN_APPROX_TC89_KCOS = 1, 2, 3, 4

__all__ = ["DetectTrails", "process_field", "process_fields_batched", "process_frame_arrays", "default_params", "measure_trail",
           "profile_row"]

_HEADER_KEYS = ("TAI", "CRPIX1", "CRPIX2", "CRVAL1", "CRVAL2", "CD1_1", "CD1_2", "CD2_1", "CD2_2")


def default_params():
    """Fresh copies of the three default dictionaries (detecttrails.py:202-239)."""
    bright = {"lwTresh": 5, "thetaTresh": 0.15, "dilateKernel": _np.ones((4, 4), _np.uint8),
              "contoursMode": RETR_LIST, "contoursMethod": CHAIN_APPROX_NONE, "minAreaRectMinLen": 1,
              "houghMethod": 20, "nlinesInSet": 3, "lineSetTresh": 0.15, "dro": 25, "debug": False}
    dim = {"minFlux": 0.02, "addFlux": 0.5, "lwTresh": 5, "thetaTresh": 0.15,
           "erodeKernel": _np.ones((3, 3), _np.uint8), "dilateKernel": _np.ones((9, 9), _np.uint8),
           "contoursMode": RETR_LIST, "contoursMethod": CHAIN_APPROX_NONE, "minAreaRectMinLen": 1,
           "houghMethod": 20, "nlinesInSet": 3, "lineSetTresh": 0.15, "dro": 20, "debug": False}
    removestars = {"pixscale": 0.396, "defaultxy": 20, "maxxy": 60,
                   "filter_caps": {'u': 22.0, 'g': 22.2, 'r': 22.2, 'i': 21.3, 'z': 20.5},
                   "magcount": 3, "maxmagdiff": 3, "debug": False}
    return bright, dim, removestars


def _rs_struct(filter, params_removestars):
    p = {k: v for k, v in params_removestars.items() if k != "debug"}
    return _native.make_rs_params(filter, **p)


def _detection(rec, shape):
    """One frame's detection record -> ``(detection, res_dict_or_None, record)``; a frame that failed on the device raises what
    the reference would have raised (detecttrails.py:126-131)."""
    status = int(rec["status"])
    if status == _native.ERR_NOLINES:
        raise TypeError("'NoneType' object is not subscriptable")  # HoughLines gave None
    if status:
        raise _native.NativeError(status, "frame failed on the device")
    if rec["found"]:
        # coordinates the way the reference computes them: numpy float32 scalars
        return True, dictify_hough(shape, (_np.float32(rec["rho"]), _np.float32(rec["theta"]))), rec
    return False, None, rec


def process_frame_arrays(img, cat, filter, params_bright, params_dim, params_removestars):
    """The hot part of process_field (detecttrails.py:119-131) on arrays.

    ``img``: float32 (h, w) frame, blotted in place by remove_stars like the reference;
    ``cat``: photoObj columns (dict) or None.  Returns ``(detection, res_dict_or_None, record)``.
    """
    if img.dtype != _np.float32 or not img.flags.c_contiguous:
        raise TypeError("process_frame_arrays needs a C-contiguous float32 frame")
    packed = _pack_one(cat)
    rs = _rs_struct(filter, params_removestars) if packed is not None else None
    with use_context(*img.shape) as ctx:
        rec = ctx.detect_batch(img, params_bright, params_dim, packed, rs)[0]
    return _detection(rec, img.shape)


def _frame_rounds(img, cat, filter, params_bright, params_dim, params_removestars, rounds_params):
    """``process_frame_arrays`` through ``detect_rounds``: (what it returns for record 0, (records [K], n_found, dup_of [K]))"""
    if img.dtype != _np.float32 or not img.flags.c_contiguous:
        raise TypeError("process_frame_arrays needs a C-contiguous float32 frame")
    packed = _pack_one(cat)
    rs = _rs_struct(filter, params_removestars) if packed is not None else None
    with use_context(*img.shape) as ctx:
        recs, nf, dup = ctx.detect_rounds(img, params_bright, params_dim, packed, rs, **rounds_params)
    return _detection(recs[0][0], img.shape), (recs[0], int(nf[0]), dup[0])


def _pack_one(cat):
    if cat is None or not len(cat["NOBSERVE"]):
        return None
    from .removestars import _check_finite
    _check_finite(cat)
    n = len(cat["NOBSERVE"])
    packed = {"count": _np.array([n], _np.int32)}
    for key in ("ROWC", "COLC", "PSFMAG", "PETROTH90"):
        packed[key] = _np.ascontiguousarray(cat[key], _np.float32).reshape(1, n, 5)
    for key in ("NOBSERVE", "NDETECT"):
        packed[key] = _np.ascontiguousarray(cat[key], _np.int32).reshape(1, n)
    return packed


def measure_trail(img, record, cat=None, filter=None, params_removestars=None, **params):
    """Trail profile of one frame (include/lfdmi.h: trail profiles): ``img`` in the orientation ``process_frame_arrays`` takes
    (blotted or not: remove_stars' squares of ``cat`` are left out of the samples either way), ``record`` the detection record
    it returned.  ``params``: fields of lfdmi_trail_params.  Returns (record of TRAIL_DTYPE, float32 profile [2K+1])."""
    img = _np.ascontiguousarray(img)
    if img.ndim != 2 or img.dtype not in (_np.dtype("<f4"), _np.dtype(">f4")):
        raise TypeError("measure_trail needs a 2-d float32 frame")
    packed = _pack_one(cat)
    rs = None
    if packed is not None:
        if filter is None or params_removestars is None:
            raise ValueError("a catalogue needs its filter and params_removestars")
        rs = _rs_struct(filter, params_removestars)
    with use_context(*img.shape) as ctx:
        out, prof = ctx.measure_trails(img, _np.asarray(record, _native.RESULT_DTYPE).reshape(1), packed, rs, **params)
    return out[0], prof[0]


def profile_row(key, trail, profile):
    """One profiles.txt row: ``run camcol filter field``, the scalar fields of the trail record (TRAIL_DTYPE order), then the
    2K+1 profile values; floats as ``repr`` (exact round trip)."""
    vals = []
    for name in _native.TRAIL_DTYPE.names:
        v = trail[name].item()
        vals.append(str(v) if isinstance(v, int) else repr(float(v)))
    vals += [repr(float(v)) for v in profile]
    return " ".join([" ".join(str(x) for x in key)] + vals) + "\n"


_BANKS = {}   # (device, params) -> (Context, DefocusBank): the defocus bank is built once per process


def defocus_bank(defocus_params=None, trail_params=None):
    """The process's ``DefocusBank`` for these grid / instrument params (``defocus_params``: heights, radii, seeings,
    instrument, ovs, max_shift, delta_chi2) and trail params, on its own small context of the device the shared context uses."""
    from .. import defocus
    from .processfield import _device_index
    dp, tp = dict(defocus_params or {}), dict(trail_params or {})
    key = (_device_index(), repr(sorted((k, _np.asarray(v).tolist()) for k, v in dp.items())), repr(sorted(tp.items())))
    if key not in _BANKS:
        ctx = _native.Context(key[0], 64, 64, 1)
        try:
            _BANKS[key] = (ctx, defocus.DefocusBank(ctx, **dp, **tp))
        except Exception:
            ctx.close()
            raise
    return _BANKS[key]


class _DefocusTee:
    """What the drivers write trail profiles to.  ``add`` appends the frame's ``profile_row`` to profiles.txt; with ``out``
    (defocus.txt beside it) every row is also fitted (include/lfdmi.h: defocus fit): the rows added since the last ``flush``
    are fitted in one call and their defocus rows written in the same order."""

    def __init__(self, profiles, out, defocus_params, trail_params, seeing=None):
        self.profiles, self.out = profiles, out
        self.defocus_params, self.trail_params = defocus_params, trail_params
        self.seeing = seeing                          # a ``_SeeingStage``: every fit gets its frame's seeing (NaN: free)
        self.pending = []

    def add(self, key, trail, profile):
        self.profiles.write(profile_row(key, trail, profile))
        if self.out is not None:
            self.pending.append((key, trail, profile))

    def flush(self):
        from .. import defocus
        if self.pending:
            ctx, bank = defocus_bank(self.defocus_params, self.trail_params)
            trails = _np.array([t for _, t, _ in self.pending], _native.TRAIL_DTYPE)
            see = None if self.seeing is None else [self.seeing.seeing_of(k) for k, _, _ in self.pending]
            fit = ctx.fit_defocus(bank, trails, _np.stack([p for _, _, p in self.pending]), see)
            self.out.write("".join(defocus.format_row(k, f) + "\n" for (k, _, _), f in zip(self.pending, fit)))
            self.pending = []
        self.profiles.flush()
        if self.out is not None:
            self.out.flush()


class _SkyStage:
    """The sky normalisation in front of detection for ``DetectTrails(normalize=True)`` (include/lfdmi.h: sky normalisation):
    a ``Sky`` handle per (context, shape), kept while it is large enough, and the sky.txt rows."""

    def __init__(self, out, params):
        from ..sky import as_params
        self.out, self.params, self._handles = out, as_params(params), {}

    def _handle(self, ctx, shape, n):
        key = (id(ctx), tuple(shape))
        h = self._handles.get(key)
        if h is None or h.ctx is not ctx or not h._s or h.max_frames < n:
            if h is not None:
                h.close()
            h = self._handles[key] = _native.Sky(ctx, shape, max_frames=n, **self.params)
        return h

    def batch(self, ctx, frames, shape, n, pinned=False):
        """n frames (pinned big-endian slots, or ``DeviceFrames``) -> (the handle's device buffer, sky records)"""
        h = self._handle(ctx, shape, n)
        rec = h.normalize(frames, pinned=pinned)
        return h.frames(n), rec

    def one(self, img):
        """one host frame -> (normalised float32 copy, its sky record)"""
        img = _np.ascontiguousarray(img, _np.float32)
        out = _np.empty_like(img)
        with use_context(*img.shape) as ctx:
            rec = self._handle(ctx, img.shape, 1).normalize(img, out=out)[0]
        return out, rec

    def row(self, key, rec):
        from ..sky import format_row
        self.out.write(format_row(key, rec) + "\n")

    def flush(self):
        self.out.flush()

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles = {}


class _StarsStage:
    """The source finder in front of detection for ``DetectTrails(find_stars=True)`` (include/lfdmi.h: source finder): each
    chunk's catalogue comes from the frames themselves (after the sky normalisation when that is on), and stars.txt gets a row
    per frame.  ``sigma``: the frames' sky sigma (target_sigma of the sky normalisation when that ran, else 0.025)."""

    def __init__(self, out, params, sigma):
        from ..stars import as_params
        self.out, self.params, self.sigma = out, as_params(params), float(sigma)

    def batch(self, ctx, frames, pixscale, **where):
        """the frames where the detect call will read them -> (device-resident catalogue, [(frame record, n_extended)])"""
        rec, frec = ctx.find_stars(frames, sigma=self.sigma, device_out=True, **where, **self.params)
        self.last = (rec, frec)                       # (``_SeeingStage`` measures on them)
        import torch
        n_ext = (rec.view(torch.int32).reshape(len(frec), -1, 8)[:, :, 3] & _native.STAR_EXTENDED).sum(1).cpu().numpy()
        return ctx.stars_catalog(rec, frec, pixscale, device=True), [(frec[j], int(n_ext[j])) for j in range(len(frec))]

    def one(self, img, pixscale):
        """one host frame -> (its catalogue as the per-frame dict of columns, (frame record, n_extended))"""
        from ..stars import n_extended, to_catalog
        with use_context(*img.shape) as ctx:
            rec, frec = ctx.find_stars(img, sigma=self.sigma, **self.params)
        self.last = (rec, frec)
        cat = to_catalog(rec, frec, pixscale)
        k = int(cat["count"][0])
        return {key: v[0, :k] for key, v in cat.items() if key != "count"}, (frec[0], int(n_extended(rec, frec)[0]))

    def row(self, key, frec, n_ext):
        from ..stars import format_row
        self.out.write(format_row(key, frec, n_ext) + "\n")

    def flush(self):
        self.out.flush()


class _SeeingStage:
    """The frame seeing in front of detection for ``DetectTrails(seeing=True)`` (include/lfdmi.h: frame seeing): each chunk's
    stars are measured before remove_stars blots them (after the sky normalisation when that is on), on the records the source
    finder left on the device -- ``_StarsStage``'s with ``find_stars=True``, otherwise a finder run of its own -- and seeing.txt
    gets a row per frame.  ``seeing_of(key)`` is what the defocus fits of that frame get: the width as the bank's seeing, NaN
    for a frame with too few stars or without a measurement."""

    def __init__(self, out, params, sigma, stars_params, pixscale, seeings):
        from ..psf import PsfParams, as_params
        from ..stars import as_params as stars_as_params
        self.out, self.params, self.sigma = out, as_params(params), float(sigma)
        self.stars_params, self.pixscale = stars_as_params(stars_params), float(pixscale)
        self.grid = _np.sort(_np.asarray(seeings, _np.float64).reshape(-1))
        self.full = PsfParams(**self.params)
        self.by_key = {}

    def _records(self, frec):
        from ..psf import SEEING_FEW, to_bank_seeing
        see = _np.atleast_1d(to_bank_seeing(frec["fwhm_px"], self.pixscale, self.full.win, self.grid, self.full.gap, self.full.ring))
        see = _np.where(frec["status"] == SEEING_FEW, _np.nan, see)
        return [(frec[j], float(see[j])) for j in range(len(frec))]

    def batch(self, ctx, frames, found=None, **where):
        """the frames where the detect call will read them, before it blots them -> [(frame record, seeing_arcsec)]"""
        if found is None:
            found = ctx.find_stars(frames, sigma=self.sigma, device_out=True, **where, **self.stars_params)
        return self._records(ctx.measure_seeing(frames, found[0], found[1], sigma=self.sigma, **where, **self.params)[1])

    def one(self, img, found=None):
        """one host frame, not blotted yet -> (frame record, seeing_arcsec)"""
        img = _np.ascontiguousarray(img, _np.float32)
        with use_context(*img.shape) as ctx:
            if found is None:
                found = ctx.find_stars(img, sigma=self.sigma, **self.stars_params)
            return self._records(ctx.measure_seeing(img, found[0], found[1], sigma=self.sigma, **self.params)[1])[0]

    def note(self, key, rec):
        self.by_key[tuple(key)] = rec[1]

    def seeing_of(self, key):
        return self.by_key.get(tuple(key)[:4], float("nan"))

    def row(self, key, frec, see):
        from ..psf import format_row
        self.out.write(format_row(key, frec, self.pixscale, see) + "\n")

    def flush(self):
        """after the chunk's fits: its frames' seeings are no longer needed"""
        self.out.flush()
        self.by_key = {}


class _PreviewStage:
    """The frame previews in front of detection for ``DetectTrails(previews=...)`` (include/lfdmi.h: frame previews): every
    chunk is previewed once where ``_SeeingStage`` measures, before the detect call blots it, and its images stay on the device;
    the frames that get a results.txt row (``which`` = "detections") or every frame that loaded ("all") are copied back, overlaid
    with their row's line (and the trails.txt lines with ``max_trails``) and written to ``out_dir`` under the image checker's
    name, with a previews.txt row each.  ``params``: bin, mode, lo_ppm, hi_ppm, limits (one (lo, hi) pair for every frame, with
    mode "given"), kind and softening of the stretch table or a ``lut`` of one's own, color and thick of the overlay."""

    def __init__(self, out, which, params, out_dir):
        from .. import masks, previews
        p = previews.as_params(params)
        self.out, self.which, self.out_dir = out, which, out_dir
        self.lut = p["lut"] if p.get("lut") is not None else previews.lut(p.get("kind", "asinh"), p.get("softening", 0.1))
        self.bin = int(p.get("bin", 4))
        self.call = {k: p[k] for k in ("bin", "mode", "lo_ppm", "hi_ppm", "limits") if k in p}
        self.draw = {k: p[k] for k in ("color", "thick") if k in p}
        self.half = masks.half_width(float("nan"))        # no measurement is asked for: the default band
        if out is not None:
            os.makedirs(out_dir, exist_ok=True)

    def wants(self, found):
        return self.which == "all" or bool(found)

    def batch(self, ctx, frames, **where):
        """the frames where the detect call will read them, before it blots them -> (device images [n, Hp, Wp], records)"""
        return ctx.frame_previews(frames, lut=self.lut, out_device=True, **self.call, **where)

    def one(self, img):
        """one host frame, not blotted yet -> (image, record)"""
        img = _np.ascontiguousarray(img, _np.float32)
        with use_context(*img.shape) as ctx:
            out, rec = ctx.frame_previews(img, lut=self.lut, **self.call)
        return out[0], rec[0]

    def segments(self, res, trails):
        """the lines of a frame as ``masks.SEGMENT_DTYPE``: its results row's, then the later rounds' found trails"""
        from .. import masks
        rows = [] if res is None else [(0, res["x1"], res["y1"], res["x2"], res["y2"], self.half)]
        if trails is not None:
            recs, n_found = trails[0], int(trails[1])
            rows += [(0, recs[k]["x1"], recs[k]["y1"], recs[k]["x2"], recs[k]["y2"], self.half) for k in range(1, n_found)]
        return masks.segments(rows)

    def row(self, key, gray, rec, res, trails):
        from .. import previews
        name = previews.filename(*key)
        previews.write_png(os.path.join(self.out_dir, name), previews.overlay(gray, self.segments(res, trails), self.bin, **self.draw))
        self.out.write(previews.format_row(key, self.bin, rec, name) + "\n")

    def flush(self):
        self.out.flush()


class _StreakStage:
    """The short-streak search behind detection for ``DetectTrails(streaks=True)`` (include/lfdmi.h: short-streak search): every
    chunk is searched after its detect call, while its frames are on the device and blotted by remove_stars, and streaks.txt
    gets one row per found streak.  ``params``: the fields of lfdmi_streak_params; ``sigma``: the frames' sky sigma."""

    def __init__(self, out, params, sigma):
        from ..streaks import as_params
        self.out, self.params, self.sigma = out, as_params(params), sigma

    def batch(self, ctx, frames, **where):
        """the frames where the detect call left them -> [(records [K], n_streaks)] per frame"""
        rec, ns = ctx.streak_search(frames, sigma=self.sigma, **where, **self.params)
        return [(rec[j], int(ns[j])) for j in range(len(ns))]

    def one(self, img):
        """one host frame, blotted by its detection -> (records [K], n_streaks)"""
        img = _np.ascontiguousarray(img, _np.float32)
        with use_context(*img.shape) as ctx:
            return self.batch(ctx, img)[0]

    def rows(self, key, recs, n):
        from ..streaks import format_row
        for k in range(n):
            self.out.write(format_row(key, k, recs[k]) + "\n")

    def flush(self):
        self.out.flush()


class _ShortRecord:
    """a frame's record of ``_RadonStage`` with ``short``: the record it has without (``base``), its short records [K], their
    n_lines and [(stack record, row)] per found short candidate (empty without ``prof_out``)"""
    __slots__ = ("base", "recs", "n_lines", "meas")

    def __init__(self, base, recs, n_lines, meas):
        self.base, self.recs, self.n_lines, self.meas = base, recs, n_lines, meas


class _WideRecord:
    """a frame's record of ``_RadonStage`` with ``wide``: the record it has without (``base``; a ``_ShortRecord`` with
    ``short``), its band records [K], their n_lines and [(stack record, row)] per found band (empty without ``prof_out``)"""
    __slots__ = ("base", "recs", "n_lines", "meas")

    def __init__(self, base, recs, n_lines, meas):
        self.base, self.recs, self.n_lines, self.meas = base, recs, n_lines, meas


class _RadonStage:
    """The faint-trail search behind detection for ``DetectTrails(radon=True)`` (include/lfdmi.h: faint-trail search): a
    ``Radon`` handle per (context, shape), kept while it is large enough, and the radon.txt rows.  ``sigma``: the frames' sky
    sigma (target_sigma of the sky normalisation when that ran, else 0.025).  ``lines`` = K: up to K lines per frame by peeling
    (``Radon.search_lines`` with ``lines_params``); a frame's record is then (records [K], n_lines) and every found line also
    gets a row in ``seg_out`` (radon_segments.txt).  ``prof_out`` (radon_profiles.txt; needs ``lines``): every found line's
    segment is measured where the search left the frames (include/lfdmi.h: stacked cross-sections; ``stack_params``) and a frame's
    record is (records [K], n_lines, [(stack record, row)] per found line); with ``defocus_out`` (radon_defocus.txt) the rows
    added since the last ``flush`` are fitted in one call, as ``_DefocusTee`` does for profiles.txt.  ``short``: the fields of
    lfdmi_radon_short_params (steps 10 - 12 of the definition): every frame is also searched by ``Radon.search_short``, whose
    plain records serve as the frame's one line when ``lines`` is None; a frame's record is then a ``_ShortRecord`` and every
    found short candidate gets a row in ``short_out`` (radon_short.txt).  With ``prof_out`` the short segments are measured
    too, and every row of radon_profiles.txt then ends with its source, ``lines`` or ``short`` (the defocus fit stays with the
    lines' rows).  ``wide``: the fields of lfdmi_radon_wide_params (steps 13 - 16): every frame is also searched by
    ``Radon.search_wide``, whose plain records serve as the frame's one line when ``lines`` and ``short`` are None; a frame's
    record is then a ``_WideRecord`` around the record it had, and every found band gets a row in ``wide_out``
    (radon_wide.txt).  With ``prof_out`` the bands' centre-line segments are measured too, their rows end with ``wide`` and
    the lines' rows with ``lines``.  ``null``: K, the realisations of the null peaks (include/lfdmi.h steps 17 - 20): every
    searched frame also gets the null peaks of each kind that is on (``lines``; ``short`` and ``wide`` where those are), a row
    per kind in ``null_out`` (radon_null.txt) and a row per found line in ``fap_out`` (radon_fap.txt).  ``null_scheme``: how
    the null frames are made (steps 21 - 22: "scramble", "signflip", "rowshift", "colshift").  ``rounds_out``
    (radon_null_rounds.txt; "signflip" only): every peel round k >= 1 that a frame's search of a kind ran also gets its null
    -- the frame with that search's lines 0 .. k-1 blotted -- a row there, and line k's radon_fap.txt row comes from it."""

    def __init__(self, out, params, sigma, lines=None, lines_params=None, seg_out=None, prof_out=None, stack_params=None,
                 defocus_out=None, defocus_params=None, short=None, short_out=None, lc=None, wide=None, wide_out=None, strip=None,
                 null=None, null_out=None, fap_out=None, null_scheme="scramble", rounds_out=None):
        from ..radon import as_params
        self.null, self.null_out, self.fap_out = null, null_out, fap_out
        self.null_scheme, self.rounds_out = null_scheme, rounds_out
        self.out, self.params, self.sigma, self._handles = out, as_params(params), float(sigma), {}
        self.wide, self.wide_out = (dict(wide) if wide is not None else None), wide_out
        self.lc, self.last_lc = lc, {}                # an ``_LcStage``; {position: [(record, sections)]} of the last ``batch`` / ``one``
        self.strip, self.last_strip = strip, {}       # a ``_StripStage``; {position: its items} likewise
        self.short, self.short_out = (dict(short) if short is not None else None), short_out
        self.lines, self.seg_out = lines, seg_out
        self.lines_params = dict(lines_params or {}, max_lines=lines) if lines is not None else None
        self.prof_out, self.stack_params = prof_out, dict(stack_params or {})
        self.defocus_out, self.defocus_params, self.pending = defocus_out, defocus_params, []
        self.seeing = None                            # a ``_SeeingStage``, set by the driver: the fits get their frame's seeing

    def _search(self, handle, frames, **where):
        """the records of a run of frames; with ``lc`` the found lines' light curves too, measured here, where the search and the
        stacked cross-sections left the frames (``_lc_part``: one list per frame)"""
        recs = self._search_all(handle, frames, **where)
        self._lc_part = None
        if self.lc is not None and self.lines is not None:
            try:
                self._lc_part = self.lc.radon(handle.ctx, frames, recs, **where)
            except Exception as e:  # noqa: BLE001 - the frames' errors entries; their radon rows stay
                self._lc_part = [e] * len(recs)
        self._strip_part = None
        if self.strip is not None and self.lines is not None:
            try:
                self._strip_part = self.strip.radon(handle.ctx, frames, recs, **where)
            except Exception as e:  # noqa: BLE001 - likewise
                self._strip_part = [e] * len(recs)
        return recs

    def _search_all(self, handle, frames, **where):
        if self.wide is None:
            return self._search_short(handle, frames, None, **where)
        wrecs, wnl, plain = handle.search_wide(frames, sigma=self.sigma, plain=True, **self.wide, **where)
        base = self._search_short(handle, frames, plain, **where)
        meas = [[] for _ in range(len(wnl))]
        if self.prof_out is not None:
            from ..stack import segments_from_radon_wide
            segs, where_ = segments_from_radon_wide(wrecs, wnl)
            if len(segs):
                srec, rows = handle.ctx.stack_profiles(frames, segs, sigma=self.sigma, **where, **self.stack_params)
                for (j, _), r, row in zip(where_, srec, rows):
                    meas[j].append((r, row))
        return [_WideRecord(base[j], wrecs[j], int(wnl[j]), meas[j]) for j in range(len(wnl))]

    def _search_short(self, handle, frames, plain, **where):
        """the records without ``wide``; plain: the wide call's plain records, which save the plain search its transform"""
        if self.short is None:
            return plain if plain is not None and self.lines is None else self._search_lines(handle, frames, **where)
        srecs, snl, plain = handle.search_short(frames, sigma=self.sigma, plain=True, **self.short, **where)
        base = plain if self.lines is None else self._search_lines(handle, frames, **where)
        meas = [[] for _ in range(len(snl))]
        if self.prof_out is not None:
            from ..stack import segments_from_radon_lines
            segs, where_ = segments_from_radon_lines(srecs, snl)
            if len(segs):
                srec, rows = handle.ctx.stack_profiles(frames, segs, sigma=self.sigma, **where, **self.stack_params)
                for (j, _), r, row in zip(where_, srec, rows):
                    meas[j].append((r, row))
        return [_ShortRecord(base[j], srecs[j], int(snl[j]), meas[j]) for j in range(len(snl))]

    def _search_lines(self, handle, frames, **where):
        if self.lines is None:
            return handle.search(frames, sigma=self.sigma, **where)
        recs, nl = handle.search_lines(frames, sigma=self.sigma, **self.lines_params, **where)
        if self.prof_out is None:
            return [(recs[j], int(nl[j])) for j in range(len(nl))]
        from ..stack import segments_from_radon_lines
        segs, where_ = segments_from_radon_lines(recs, nl)
        meas = [[] for _ in range(len(nl))]
        if len(segs):
            srec, rows = handle.ctx.stack_profiles(frames, segs, sigma=self.sigma, **where, **self.stack_params)
            for (j, _), r, row in zip(where_, srec, rows):
                meas[j].append((r, row))
        return [(recs[j], int(nl[j]), meas[j]) for j in range(len(nl))]

    def _handle(self, ctx, shape, n):
        key = (id(ctx), tuple(shape))
        h = self._handles.get(key)
        if h is None or h.ctx is not ctx or not h._r or h.max_frames < n:
            if h is not None:
                h.close()
            h = self._handles[key] = _native.Radon(ctx, shape, max_frames=n, **self.params)
        return h

    def batch(self, ctx, frames, shape, todo, **where):
        """the frames ``todo`` (ascending positions in ``frames``), searched in runs of neighbours -> {position: record}"""
        out, k = {}, 0
        self.last_lc, self.last_strip = {}, {}
        while k < len(todo):
            m = k
            while m + 1 < len(todo) and todo[m + 1] == todo[m] + 1:
                m += 1
            a, b = todo[k], todo[m] + 1
            part = frames.slice(a, b) if isinstance(frames, _native.DeviceFrames) else frames[a:b]
            recs = self._search(self._handle(ctx, shape, min(b - a, 16)), part, **where)
            out.update(zip(range(a, b), recs))
            if self._lc_part is not None:
                self.last_lc.update(zip(range(a, b), self._lc_part))
            if self._strip_part is not None:
                self.last_strip.update(zip(range(a, b), self._strip_part))
            k = m + 1
        return out

    def one(self, img):
        """one host frame -> its record"""
        img = _np.ascontiguousarray(img, _np.float32)
        with use_context(*img.shape) as ctx:
            rec = self._search(self._handle(ctx, img.shape, 1), img)[0]
        self.last_lc = {0: self._lc_part[0]} if self._lc_part is not None else {}
        self.last_strip = {0: self._strip_part[0]} if self._strip_part is not None else {}
        return rec

    def null_kinds(self):
        """[(kind, its parameters)] of the null peaks: the searches that are on"""
        return [("lines", {})] + ([("short", self.short)] if self.short is not None else []) + \
            ([("wide", self.wide)] if self.wide is not None else [])

    def peeled_lines(self, rec):
        """{kind: (records [max_lines], n_lines)} of a frame's record: what the peeling searches that are on found"""
        out = {}
        if isinstance(rec, _WideRecord):
            out["wide"] = (rec.recs, rec.n_lines)
            rec = rec.base
        if isinstance(rec, _ShortRecord):
            out["short"] = (rec.recs, rec.n_lines)
            rec = rec.base
        if self.lines is not None:
            out["lines"] = (rec[0], rec[1])
        return out

    def null_batch(self, ctx, frames, shape, todo, seeds, recs=None, **where):
        """the null peaks of the frames ``todo`` (as in ``batch``; seeds: one per entry of todo), where the search left the
        frames -> {position: {kind: float32 [K]}}; with ``rounds_out`` and the frames' records ``recs`` ({position: record})
        also "rounds": {kind: {k: float32 [K]}} for the rounds k >= 1 the kind's search ran on the frame"""
        from ..radon import peel_from_lines
        out, k = {}, 0
        while k < len(todo):
            m = k
            while m + 1 < len(todo) and todo[m + 1] == todo[m] + 1:
                m += 1
            a, b = todo[k], todo[m] + 1
            part = frames.slice(a, b) if isinstance(frames, _native.DeviceFrames) else frames[a:b]
            handle = self._handle(ctx, shape, min(b - a, 16))
            for kind, kp in self.null_kinds():
                if kind == "lines" and self.rounds_out is not None and self.lines is not None:
                    kp = self.lines_params                # (its peel_halfwidth is the rounds')
                snr = handle.null(part, K=self.null, kind=kind, sigma=self.sigma, seeds=seeds[k:m + 1], scheme=self.null_scheme, **kp,
                                  **where)["snr"]
                for j in range(a, b):
                    out.setdefault(j, {})[kind] = _np.array(snr[j - a], _np.float32)
                if self.rounds_out is None or recs is None:
                    continue
                # every frame of the run goes through every round some frame ran; a frame keeps the rounds it ran itself
                found = [self.peeled_lines(recs[j]).get(kind) for j in range(a, b)]
                if any(f is None for f in found):
                    continue
                lines, nl = _np.stack([f[0] for f in found]), _np.array([f[1] for f in found])
                ran = _np.minimum(nl, lines.shape[1] - 1)        # the last round a frame ran
                for rnd in range(1, int(ran.max()) + 1):
                    snr = handle.null(part, K=self.null, kind=kind, sigma=self.sigma, seeds=seeds[k:m + 1], scheme="signflip",
                                      peel=peel_from_lines(lines, nl, rnd), **kp, **where)["snr"]
                    for j in range(a, b):
                        if rnd <= ran[j - a]:
                            out[j].setdefault("rounds", {}).setdefault(kind, {})[rnd] = _np.array(snr[j - a], _np.float32)
            k = m + 1
        return out

    def null_one(self, img, seed, rec=None):
        """one host frame (and its record) -> its {kind: float32 [K]}"""
        img = _np.ascontiguousarray(img, _np.float32)
        with use_context(*img.shape) as ctx:
            return self.null_batch(ctx, img[None], img.shape, [0], [seed], None if rec is None else {0: rec})[0]

    def found_lines(self, rec):
        """{kind: [(place in peel order, snr)]} of a frame's record: the lines that have rows in the kinds' files"""
        out = {}
        if isinstance(rec, _WideRecord):
            out["wide"] = [(k, rec.recs[k]["snr"]) for k in range(rec.n_lines)]
            rec = rec.base
        if isinstance(rec, _ShortRecord):
            out["short"] = [(k, rec.recs[k]["snr"]) for k in range(rec.n_lines)]
            rec = rec.base
        if self.lines is None:
            out["lines"] = [(0, rec["snr"])] if int(rec["found"]) else []
        else:
            out["lines"] = [(k, rec[0][k]["snr"]) for k in range(rec[1])]
        return out

    def null_rows(self, key, rec, nulls):
        """a frame's radon_null.txt rows, one per kind, and its radon_fap.txt rows, one per found line"""
        from ..radon import format_fap_row, format_null_row, format_null_rounds_row
        found = self.found_lines(rec)
        for kind, _ in self.null_kinds():
            self.null_out.write(format_null_row(key, kind, nulls[kind]) + "\n")
            rounds = nulls.get("rounds", {}).get(kind, {})
            for k in sorted(rounds):
                self.rounds_out.write(format_null_rounds_row(key, kind, k, rounds[k]) + "\n")
            for k, snr in found.get(kind, []):                   # (line k was found in round k: its null is that round's)
                self.fap_out.write(format_fap_row(key, kind, k, snr, rounds.get(k, nulls[kind])) + "\n")

    def row(self, key, rec):
        """the rows of one frame's record: the line if it was found; with ``lines``, every found line in peel order"""
        from ..radon import format_row, format_segment_row
        tag = ""
        if isinstance(rec, _WideRecord):
            from ..radon import format_wide_row
            from ..stack import format_row as format_profile_row
            tag = " lines"
            for k in range(rec.n_lines):
                self.wide_out.write(format_wide_row(key, k, rec.recs[k]) + "\n")
            for k, (srec, _) in enumerate(rec.meas):
                self.prof_out.write(format_profile_row(key, k, srec) + " wide\n")
            rec = rec.base
        if isinstance(rec, _ShortRecord):
            from ..radon import format_short_row
            from ..stack import format_row as format_profile_row
            tag = " lines"
            for k in range(rec.n_lines):
                self.short_out.write(format_short_row(key, k, rec.recs[k]) + "\n")
            for k, (srec, _) in enumerate(rec.meas):
                self.prof_out.write(format_profile_row(key, k, srec) + " short\n")
            rec = rec.base
        if self.lines is None:
            if int(rec["found"]):
                self.out.write(format_row(key, rec) + "\n")
            return
        recs, nl = rec[:2]
        for k in range(nl):
            self.out.write(format_row(key, recs[k]) + "\n")
            self.seg_out.write(format_segment_row(key, k, recs[k]) + "\n")
        if self.prof_out is not None:
            from ..stack import format_row as format_profile_row
            for k, (srec, prow) in enumerate(rec[2]):
                self.prof_out.write(format_profile_row(key, k, srec) + tag + "\n")
                if self.defocus_out is not None:
                    self.pending.append(((*key, k), srec, prow))

    def flush(self):
        self.out.flush()
        if self.seg_out is not None:
            self.seg_out.flush()
        if self.short_out is not None:
            self.short_out.flush()
        if self.wide_out is not None:
            self.wide_out.flush()
        if self.null_out is not None:
            self.null_out.flush()
            self.fap_out.flush()
        if self.rounds_out is not None:
            self.rounds_out.flush()
        if self.prof_out is not None:
            self.prof_out.flush()
        if self.defocus_out is not None:
            if self.pending:
                from .. import defocus
                from ..stack import to_trails
                tp = {"prof_half": self.stack_params.get("prof_half", 24.0), "prof_step": self.stack_params.get("step", 0.5),
                      "wing": self.stack_params.get("wing", 8), "pixscale": self.stack_params.get("pixscale", 0.396)}
                ctx, bank = defocus_bank(self.defocus_params, tp)
                trails = to_trails(_np.array([r for _, r, _ in self.pending], _native.STACK_DTYPE))
                see = None if self.seeing is None else [self.seeing.seeing_of(k) for k, _, _ in self.pending]
                fit = ctx.fit_defocus(bank, trails, _np.stack([p for _, _, p in self.pending]), see)
                self.defocus_out.write("".join(defocus.format_row(k, f) + "\n" for (k, _, _), f in zip(self.pending, fit)))
                self.pending = []
            self.defocus_out.flush()

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles = {}


class _MaskStage:
    """The trail masks behind the measurements for ``DetectTrails(trail_masks=True)`` (include/lfdmi.h: trail masks): one
    masks.txt row per results.txt row (source ``detect``) and, with ``radon_lines``, per found faint line (source ``radon``),
    and with ``mask_dir`` the frame's packed plane.  ``half_params``: keywords of ``masks.half_width``.  A frame's segments are
    flagged in one mask-only call on the shared context when its rows are written."""

    def __init__(self, out, half_params=None, mask_dir=None):
        self.out, self.half_params, self.mask_dir = out, dict(half_params or {}), mask_dir
        if mask_dir is not None:
            os.makedirs(mask_dir, exist_ok=True)

    def detect_segment(self, res, meas):
        """(x1, y1, x2, y2, half) of a detected frame: the refined extent and the fwhm of its trail record where the measurement
        is OK, else the results row's points (far off the image: the whole line) and the default half-width"""
        from ..masks import half_width
        if isinstance(meas, tuple) and int(meas[0]["status"]) == _native.TRAIL_OK:
            t = meas[0]
            return (float(t["x1"]), float(t["y1"]), float(t["x2"]), float(t["y2"]), half_width(float(t["fwhm"]), **self.half_params))
        fwhm = float(meas[0]["fwhm"]) if isinstance(meas, tuple) else float("nan")
        return (float(res["x1"]), float(res["y1"]), float(res["x2"]), float(res["y2"]), half_width(fwhm, **self.half_params))

    def radon_segments(self, line):
        """[(x1, y1, x2, y2, half)] of a frame's found faint lines (a ``_RadonStage`` record with ``lines``), in peel order; the
        half-width from the stacked cross-section's fwhm where that was measured and is OK"""
        from ..masks import half_width
        while isinstance(line, (_ShortRecord, _WideRecord)):
            line = line.base
        if not isinstance(line, tuple):
            return []
        recs, nl = line[:2]
        out = []
        for k in range(nl):
            fwhm = float("nan")
            if len(line) > 2 and k < len(line[2]) and int(line[2][k][0]["status"]) == _native.STACK_OK:
                fwhm = float(line[2][k][0]["fwhm"])
            r = recs[k]
            out.append((float(r["ex1"]), float(r["ey1"]), float(r["ex2"]), float(r["ey2"]), half_width(fwhm, **self.half_params)))
        return out

    def rows(self, key, shape, source, segs):
        """flags ``segs`` on one plane of ``shape`` and writes their rows (and the plane)"""
        from .. import masks
        if not segs:
            return
        sg = masks.segments([(0, *s) for s in segs])
        with use_context(*shape) as ctx:
            mask, stats, _ = ctx.mask_trails(None, sg, shape=tuple(shape))
        for k, s in enumerate(sg):
            self.out.write(masks.format_row(key, source, k, s, stats[k]["n_pix"]) + "\n")
        if self.mask_dir is not None:
            bits, shp = masks.pack(mask)
            _np.savez(os.path.join(self.mask_dir, "mask-%s-%s-%s-%s.npz" % tuple(key)), bits=bits, shape=_np.array(shp, _np.int64))

    def flush(self):
        self.out.flush()


class _RoundsStage:
    """Several trails per frame for ``DetectTrails(max_trails=K)`` (include/lfdmi.h: detection rounds): the chunk's detect call
    becomes ``detect_rounds`` with ``params`` (record 0 serves everything the plain record served), and every found trail of a
    frame, round 0 included, gets its row in trails.txt."""

    def __init__(self, out, params):
        self.out, self.params = out, dict(params)

    def rows(self, key, recs, n_found, dup_of):
        from ..rounds import format_row
        for k in range(int(n_found)):
            self.out.write(format_row(key, k, recs[k], dup_of[k]) + "\n")

    def flush(self):
        self.out.flush()


class _LcStage:
    """The light curves behind the measurements for ``DetectTrails(light_curves=True)`` (include/lfdmi.h: light curves): every
    results.txt row (source ``detect``) and, with ``radon_lines``, every found faint line (source ``radon``) is measured in
    sections where its frames are still alive -- beside ``measure_trails`` and beside ``stack_profiles``, on the buffer those
    read -- and kept in the chunk's slot until ``_emit`` writes one lightcurves.txt row per section that is not EMPTY and one
    lightcurve_summary.txt row per segment.  The segments are the trail masks' (``_MaskStage.detect_segment`` /
    ``radon_segments`` with ``half_params``), with the sky bands of ``lightcurve.segments``.  ``sigma``: the frames' sky sigma."""

    def __init__(self, out, summary_out, params, sigma, half_params=None, max_sections=256):
        from ..lightcurve import as_params
        self.out, self.summary_out, self.params, self.sigma = out, summary_out, as_params(params), float(sigma)
        self.max_sections = int(max_sections)
        self.segs = _MaskStage(None, half_params)       # (the half-width rule and the segments of a record stay in one place)

    def measure(self, ctx, frames, rows, **where):
        """(frame, x1, y1, x2, y2, half) rows on ``frames`` -> [(record, its sections)] in the rows' order"""
        from .. import lightcurve
        if not rows:
            return []
        rec, sec = ctx.light_curves(frames, lightcurve.segments(rows), sigma=self.sigma, max_sections=self.max_sections, **where,
                                    **self.params)
        return [(rec[k], sec[k]) for k in range(len(rows))]

    def radon(self, ctx, frames, lines, **where):
        """a run of frames and their ``_RadonStage`` records -> per frame the [(record, sections)] of its found lines"""
        rows, owner = [], []
        for j, line in enumerate(lines):
            for s in self.segs.radon_segments(line):
                rows.append((j, *s))
                owner.append(j)
        out = [[] for _ in lines]
        for j, item in zip(owner, self.measure(ctx, frames, rows, **where)):
            out[j].append(item)
        return out

    def rows(self, key, source, items):
        from .. import lightcurve
        for k, (rec, sec) in enumerate(items):
            text = lightcurve.format_rows(key, source, k, rec, sec)
            if text:
                self.out.write("\n".join(text) + "\n")
            self.summary_out.write(lightcurve.format_summary_row(key, source, k, rec) + "\n")

    def flush(self):
        self.out.flush()
        self.summary_out.flush()


class _StripStage:
    """The trail strips behind the measurements for ``DetectTrails(trail_strips=True)`` (include/lfdmi.h: trail strips): the
    segments ``_LcStage`` measures, at the same places, each half-width widened by ``wing`` so that the wings are sky
    (``strips.segments_from_mask_segments``' rule), kept in the chunk's slot until ``_emit`` writes one strips.txt row per section
    that is not EMPTY and, with ``strips_dir``, the segment's maps (.npz) and preview (.png).  ``sigma``: the frames' sky sigma."""

    def __init__(self, out, params, sigma, half_params=None, strips_dir=None, max_sections=1024):
        from ..strips import DEFAULT_WING, as_params
        self.out, self.params, self.sigma, self.strips_dir = out, as_params(params), float(sigma), strips_dir
        self.wing = float(self.params.get("wing", DEFAULT_WING))
        self.max_sections = int(max_sections)             # (a results row reaches about 1000 px past the frame: 512 sections of 8 px)
        self.segs = _MaskStage(None, half_params)
        if strips_dir is not None:
            os.makedirs(strips_dir, exist_ok=True)

    def measure(self, ctx, frames, rows, **where):
        """(frame, x1, y1, x2, y2, half) rows on ``frames`` -> [(record, its sections, its maps, its segment)] in the rows' order"""
        from .. import strips
        if not rows:
            return []
        segs = strips.segments([(*r[:5], float(r[5]) + self.wing) for r in rows])
        rec, sec, cells = ctx.trail_strips(frames, segs, sigma=self.sigma, max_sections=self.max_sections, **where, **self.params)
        return [(rec[k], sec[k], strips.maps(rec[k], cells[k]), segs[k]) for k in range(len(rows))]

    def radon(self, ctx, frames, lines, **where):
        """a run of frames and their ``_RadonStage`` records -> per frame the items of its found lines"""
        rows, owner = [], []
        for j, line in enumerate(lines):
            for s in self.segs.radon_segments(line):
                rows.append((j, *s))
                owner.append(j)
        out = [[] for _ in lines]
        for j, item in zip(owner, self.measure(ctx, frames, rows, **where)):
            out[j].append(item)
        return out

    def rows(self, key, source, items):
        from .. import strips
        for k, (rec, sec, maps, seg) in enumerate(items):
            text = strips.format_rows(key, source, k, rec, sec)
            if text:
                self.out.write("\n".join(text) + "\n")
            if self.strips_dir is not None:
                stem = os.path.join(self.strips_dir, "strip-%s-%s-%s-%s-%s%d" % (*key, source, k))
                _np.savez(stem + ".npz", mean=maps["mean"], n=maps["n"], n_geom=maps["n_geom"],
                          segment=_np.array([float(seg[f]) for f in ("x1", "y1", "x2", "y2", "half")]))
                strips.write_png(stem + ".png", maps["mean"])

    def flush(self):
        self.out.flush()


@contextlib.contextmanager
def _both(a, b):
    """two context managers as one (``process`` is at Python's limit of nested blocks)"""
    with a as x, b as y:
        yield x, y


class _DevView:
    """device frames as something ``torch.as_tensor`` can look at without a copy"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


class _SubStage:
    """The trail subtraction for ``DetectTrails(subtract_trails=True)`` (include/lfdmi.h: trail subtraction): the segments
    ``_LcStage`` and ``_StripStage`` measure, each half-width widened by ``wing``, modelled and taken out of the chunk's frames
    after every other measurement, because it changes them.  Frames on the device change where they are; the loader's pinned
    big-endian slots are left alone and the frames that carry a segment are cleaned as native copies.  The chunk's slot keeps
    (source, [(record, segment)], the cleaned frame if ``clean_dir``) until ``_emit`` writes one subtracted.txt row per segment
    and, with ``clean_dir``, the frame as clean-<run>-<camcol>-<filter>-<field>.npz."""

    def __init__(self, out, params, half_params=None, clean_dir=None, max_sections=1024):
        from ..subtract import DEFAULT_WING, as_params
        self.out, self.params, self.clean_dir = out, as_params(params), clean_dir
        if not int(self.params.get("apply", 1)):
            raise ValueError("sub_params: apply=0 subtracts nothing; leave subtract_trails off instead")
        self.wing = float(self.params.get("wing", DEFAULT_WING))
        self.max_sections = int(max_sections)             # (a results row reaches about 1000 px past the frame)
        self.segs = _MaskStage(None, half_params)
        if clean_dir is not None:
            os.makedirs(clean_dir, exist_ok=True)

    def run(self, ctx, frames, per_frame, **where):
        """per_frame: {frame index j: (source, [(x1, y1, x2, y2, half)])} on ``frames`` -> {j: (source, [(record, segment)],
        cleaned frame or None)}"""
        from .. import _native, subtract
        js = sorted(j for j in per_frame if per_frame[j][1])
        if not js:
            return {}
        host_be = isinstance(frames, _np.ndarray) and frames.dtype != _np.float32
        if host_be:                                       # native copies of the frames that carry a segment
            work, at, where = _np.ascontiguousarray(frames[js], _np.float32), {j: k for k, j in enumerate(js)}, {}
        else:
            work, at = frames, {j: j for j in js}
        rows = [(at[j], *seg[:4], float(seg[4]) + self.wing) for j in js for seg in per_frame[j][1]]
        segs = subtract.segments(rows)
        rec, _ = ctx.subtract_trails(work, segs, max_sections=self.max_sections, **where, **self.params)
        out, k = {}, 0
        for j in js:
            n = len(per_frame[j][1])
            clean = None
            if self.clean_dir is not None:
                if isinstance(work, _np.ndarray):
                    clean = _np.array(work[at[j]], _np.float32)
                elif isinstance(work, _native.DeviceFrames):
                    import torch
                    view = torch.as_tensor(_DevView(work.address_of(j), work.shape[1:]), device="cuda")
                    clean = view.cpu().numpy()
                else:
                    clean = work[j].cpu().numpy()
            out[j] = (per_frame[j][0], [(rec[k + m], segs[k + m]) for m in range(n)], clean)
            k += n
        return out

    def rows(self, key, source, items, clean):
        from .. import subtract
        for k, (rec, seg) in enumerate(items):
            self.out.write("\n".join(subtract.format_rows(key, source, k, rec)) + "\n")
        if self.clean_dir is not None and clean is not None:
            _np.savez(os.path.join(self.clean_dir, "clean-%s-%s-%s-%s.npz" % tuple(key)), frame=clean,
                      segments=_np.array([[float(seg[f]) for f in ("x1", "y1", "x2", "y2", "half")] for _, seg in items]))

    def flush(self):
        self.out.flush()


def _load_frame(run, camcol, filter, field, catalog=True):
    """Frame image (float32, C-contiguous), results-row head, photoObj columns; raises like the
    reference when neither the .fits nor the .fits.bz2 exists (detecttrails.py:81-87)."""
    path = sdssfiles.filename("frame", run=run, camcol=camcol, field=field, filter=filter)
    if not os.path.exists(path):
        if not os.path.exists(path + ".bz2"):
            raise FileNotFoundError(("File {0} or its bz2 compressed version not found. "
                                     "Are you sure they exist?").format(path))
        path = path + ".bz2"  # decompressed in memory; no $FITS_DUMP round trip needed
    img, h = fitslite.read_image(path)
    img = _np.ascontiguousarray(img, dtype=_np.float32)
    head = " ".join(str(x) for x in (run, camcol, filter, field, *(h[k] for k in _HEADER_KEYS)))
    cat = read_photoObj_arrays(sdssfiles.filename("photoObj", run=run, camcol=camcol, field=field)) if catalog else None
    return img, head, cat


def _log_error(errors, ids, exc, debug):
    """errors.txt entry of the reference (detecttrails.py:133-139): ids, 3-frame traceback, message."""
    if debug:
        traceback.print_exception(type(exc), exc, exc.__traceback__, limit=3)
    errors.write("{} {} {} {}\n".format(*ids))
    traceback.print_exception(type(exc), exc, exc.__traceback__, limit=3, file=errors)
    errors.write(str(exc) + "\n\n")


def _load_many(ids):
    """[(key, img, head, cat) or (key, exception)] for every key, in order (FITS / bz2 decoding: host work that
    DetectTrails.process overlaps with the GPU passes of the previous chunk)."""
    out = []
    for key in ids:
        try:
            out.append((key,) + _load_frame(*key))
        except Exception as e:  # noqa: BLE001
            out.append((key, e))
    return out


def _frame_shape(keys):
    """(h, w) of the first frame of the selection that can be opened (SDSS frames are all 1489 x 2048; a selection none of
    whose files exists gets the SDSS shape and one errors entry per frame)."""
    for key in keys[:64]:
        run, camcol, flt, field = key
        try:
            path = sdssfiles.filename("frame", run=run, camcol=camcol, field=field, filter=flt)
            if os.path.exists(path):
                with open(path, "rb") as f:
                    head = f.read(16 * fitslite.BLOCK)
            elif os.path.exists(path + ".bz2"):
                with bz2.open(path + ".bz2", "rb") as f:
                    head = f.read(16 * fitslite.BLOCK)
            else:
                continue
            end = header_end(head)
            if end > 0 and card_value(head[:end], b"NAXIS") == 2:
                return int(card_value(head[:end], b"NAXIS2")), int(card_value(head[:end], b"NAXIS1"))
        except Exception:  # noqa: BLE001 - the frame's own error is logged when its turn comes
            continue
    return 1489, 2048


class _Chunk:
    """What one driver call runs with -- the output files, the three parameter dictionaries, the profiles sink (``add(key, trail,
    profile)``) with its trail params, the ``_SkyStage`` -- and the per-frame slots of its ``n`` frames: ``rows[i]`` the
    detection record, what ``process_frame_arrays`` returned, or the exception that is the frame's errors entry; ``meas[i]``
    (trail record, profile) or the measurement's exception; ``srecs[i]`` the sky record if the frame was normalised;
    ``rlines[i]`` the faint-trail record of a frame without a detection (``radon``: a ``_RadonStage``), or its exception.  A new
    per-frame product gets a slot here, a step in ``_run_group`` and ``_run_frame``, and its row in ``_emit``."""

    def __init__(self, n, results, errors, params_bright, params_dim, params_removestars, profiles, trail_params, sky, radon=None,
                 stars=None, masks=None, lc=None, strip=None, sub=None, seeing=None, rounds=None, preview=None, streak=None):
        self.streak = streak                          # a ``_StreakStage``; ``streaks[i]``: (records [K], n_streaks) or the exception
        self.streaks = [None] * n
        self.preview = preview                        # a ``_PreviewStage``; ``previews[i]``: (image, record) or the exception
        self.previews = [None] * n
        self.results, self.errors, self.profiles, self.sky, self.radon, self.stars = results, errors, profiles, sky, radon, stars
        self.rounds = rounds                          # a ``_RoundsStage``; ``trails[i]``: (records [K], n_found, dup_of [K])
        self.trails = [None] * n
        self.seeing = seeing                          # a ``_SeeingStage``; ``seerecs[i]``: (frame record, seeing_arcsec) or the exception
        self.seerecs = [None] * n
        self.sub = sub                                # a ``_SubStage``; ``subs[i]``: (source, [(record, segment)], frame) or the exception
        self.subs = [None] * n
        self.masks = masks                            # a ``_MaskStage``: its rows are made in ``_emit``, from the slots below
        self.lc = lc                                  # a ``_LcStage``; ``lcs[i]``: (source, [(record, sections)]) or the exception
        self.lcs = [None] * n
        self.strip = strip                            # a ``_StripStage``; ``strips[i]``: (source, its items) or the exception
        self.strips = [None] * n
        self.shapes = [None] * n                      # the shape of a frame that ran on its own
        self.strecs = [None] * n                      # (frame record, n_extended) of the source finder (``stars``: a ``_StarsStage``)
        self.params_bright, self.params_dim, self.params_removestars = params_bright, params_dim, params_removestars
        self.trail_params = trail_params or {}
        self.debug = params_bright.get("debug") or params_dim.get("debug")
        self.rows, self.meas, self.srecs, self.rlines = [None] * n, [None] * n, [None] * n, [None] * n
        self.keys = [None] * n                        # (run, camcol, filter, field): the seed of a frame's null peaks
        self.nulls = [None] * n                       # {kind: null peaks} of a searched frame (``radon`` with ``null``), or the exception
        self.gpu_s = 0.0                              # inside the sky + detect calls of the groups that went through


def _sub_segments(c, i, detection, res, line):
    """frame i's segments for the subtraction: (source, [(x1, y1, x2, y2, half)]), the trail masks' of its results row or of its
    found faint lines"""
    if detection:
        return "detect", [c.sub.segs.detect_segment(res, c.meas[i])]
    if line is not None and not isinstance(line, Exception):
        return "radon", list(c.sub.segs.radon_segments(line))
    return "detect", []


def _run_frame(c, i, filter, frame):
    """Frame i on its own, under its own try: ``frame()`` -> (float32 img, cat); sky normalisation if on, detection, and the
    trail measurement of a detected frame."""
    c.lcs[i] = c.strips[i] = c.subs[i] = c.trails[i] = c.previews[i] = c.streaks[i] = None
    try:
        img, cat = frame()
        c.shapes[i] = tuple(img.shape)
        if c.sky is not None:
            img, c.srecs[i] = c.sky.one(img)
        if c.stars is not None:
            cat, c.strecs[i] = c.stars.one(img, c.params_removestars["pixscale"])
        if c.seeing is not None:                      # before the frame is blotted
            try:
                c.seerecs[i] = c.seeing.one(img, c.stars.last if c.stars is not None else None)
                c.seeing.note(c.keys[i], c.seerecs[i])
            except Exception as e:  # noqa: BLE001
                c.seerecs[i] = e
        if c.preview is not None:                     # likewise
            try:
                c.previews[i] = c.preview.one(img)
            except Exception as e:  # noqa: BLE001
                c.previews[i] = e
        if c.rounds is not None:
            c.rows[i], c.trails[i] = _frame_rounds(img, cat, filter, c.params_bright, c.params_dim, c.params_removestars, c.rounds.params)
        else:
            c.rows[i] = process_frame_arrays(img, cat, filter, c.params_bright, c.params_dim, c.params_removestars)
        if c.preview is not None and not c.preview.wants(c.rows[i][0]):
            c.previews[i] = None
        if c.profiles is not None and c.rows[i][0]:
            try:
                c.meas[i] = measure_trail(img, c.rows[i][2], cat, filter, c.params_removestars, **c.trail_params)
            except Exception as e:  # noqa: BLE001
                c.meas[i] = e
        if c.lc is not None and c.rows[i][0]:
            try:
                fr = _np.ascontiguousarray(img, _np.float32)
                with use_context(*fr.shape) as ctx:
                    c.lcs[i] = ("detect", c.lc.measure(ctx, fr, [(0, *c.lc.segs.detect_segment(c.rows[i][1], c.meas[i]))]))
            except Exception as e:  # noqa: BLE001
                c.lcs[i] = e
        if c.strip is not None and c.rows[i][0]:
            try:
                fr = _np.ascontiguousarray(img, _np.float32)
                with use_context(*fr.shape) as ctx:
                    c.strips[i] = ("detect", c.strip.measure(ctx, fr, [(0, *c.strip.segs.detect_segment(c.rows[i][1], c.meas[i]))]))
            except Exception as e:  # noqa: BLE001
                c.strips[i] = e
        if c.radon is not None and not c.rows[i][0]:
            try:
                c.rlines[i] = c.radon.one(img)
                if 0 in c.radon.last_lc:
                    lc = c.radon.last_lc[0]
                    c.lcs[i] = lc if isinstance(lc, Exception) else ("radon", lc)
                if 0 in c.radon.last_strip:
                    st = c.radon.last_strip[0]
                    c.strips[i] = st if isinstance(st, Exception) else ("radon", st)
            except Exception as e:  # noqa: BLE001
                c.rlines[i] = e
            if c.radon.null is not None and not isinstance(c.rlines[i], Exception):
                try:
                    from ..radon import null_seed
                    c.nulls[i] = c.radon.null_one(img, null_seed(*c.keys[i]), c.rlines[i])
                except Exception as e:  # noqa: BLE001
                    c.nulls[i] = e
        if c.streak is not None:                      # the frame as its detection left it
            try:
                c.streaks[i] = c.streak.one(img)
            except Exception as e:  # noqa: BLE001
                c.streaks[i] = e
        if c.sub is not None:                         # last: it changes the frame (a copy of it here)
            try:
                todo = _sub_segments(c, i, c.rows[i][0], c.rows[i][1], c.rlines[i])
                if todo[1]:
                    fr = _np.array(img, _np.float32, order="C")
                    with use_context(*fr.shape) as ctx:
                        c.subs[i] = c.sub.run(ctx, fr[None], {0: todo}).get(0)
            except Exception as e:  # noqa: BLE001
                c.subs[i] = e
    except Exception as e:  # noqa: BLE001 - the reference swallows everything per frame
        c.rows[i] = e


def _run_group(c, idx, filter, shape, inflight, source, second, detect_kw=None, measure_kw=None):
    """The frames ``idx`` of one filter and shape in ONE lfdmi_detect_batch call (frames with different filters use different
    magnitude caps).  ``source()`` -> (frames, padded catalogue arrays); ``detect_kw`` / ``measure_kw`` say where those frames
    are (``pinned``, ``native_device``).  With sky on the frames are normalised into the handle's device buffer first (the upload
    happens there) and detection and measurement read that buffer.  A measurement that fails is the error of every detected
    frame of the group.  A call-level failure: every frame on its own (``_run_frame``) from ``second(i)`` -> (img, cat);
    ``second`` None: the frames are wherever the failed call left them, and each of them logs the call's exception."""
    import time
    detect_kw, measure_kw = detect_kw or {}, measure_kw or {}
    try:
        frames, packed = source()
        rs = _rs_struct(filter, c.params_removestars)
        with use_context(*shape, inflight=inflight) as ctx:
            t0 = time.perf_counter()
            if c.sky is not None:
                frames, srecs = c.sky.batch(ctx, frames, shape, len(idx), pinned=detect_kw.get("pinned", False))
                for j, i in enumerate(idx):
                    c.srecs[i] = srecs[j]
                detect_kw = measure_kw = {}
            if c.stars is not None:                   # the chunk's catalogue: the sources of the frames the detect call reads
                packed, strecs = c.stars.batch(ctx, frames, rs.pixscale, **detect_kw)
                for j, i in enumerate(idx):
                    c.strecs[i] = strecs[j]
            if c.seeing is not None:                  # before the detect call blots the frames
                try:
                    seerecs = c.seeing.batch(ctx, frames, c.stars.last if c.stars is not None else None, **detect_kw)
                    for j, i in enumerate(idx):
                        c.seerecs[i] = seerecs[j]
                        c.seeing.note(c.keys[i], seerecs[j])
                except Exception as e:  # noqa: BLE001
                    for i in idx:
                        c.seerecs[i] = e
            pv = None
            if c.preview is not None:                 # likewise; the images stay on the device until the records say which are wanted
                try:
                    pv = c.preview.batch(ctx, frames, **detect_kw)
                except Exception as e:  # noqa: BLE001
                    pv = e
            if c.rounds is not None:
                all_recs, nf, dup = ctx.detect_rounds(frames, c.params_bright, c.params_dim, packed, rs, **detect_kw, **c.rounds.params)
                recs = _np.ascontiguousarray(all_recs[:, 0])
                for j, i in enumerate(idx):
                    c.trails[i] = (all_recs[j], int(nf[j]), dup[j])
            else:
                recs = ctx.detect_batch(frames, c.params_bright, c.params_dim, packed, rs, **detect_kw)
            c.gpu_s += time.perf_counter() - t0
            if pv is not None:
                for j, r in enumerate(recs):
                    if c.preview.wants(not int(r["status"]) and int(r["found"])):
                        c.previews[idx[j]] = pv if isinstance(pv, Exception) else (pv[0][j].cpu().numpy(), pv[1][j])
            if c.profiles is not None:
                try:
                    trails, profs = ctx.measure_trails(frames, recs, packed, rs, **measure_kw, **c.trail_params)
                    for j, i in enumerate(idx):
                        c.meas[i] = (trails[j], profs[j])
                except Exception as e:  # noqa: BLE001
                    for i in idx:
                        c.meas[i] = e
            if c.lc is not None:                      # the detected frames, on the buffer the measurement read
                found = [j for j, r in enumerate(recs) if not int(r["status"]) and int(r["found"])]
                try:
                    rows = [(j, *c.lc.segs.detect_segment(_detection(recs[j], shape)[1], c.meas[idx[j]])) for j in found]
                    for j, item in zip(found, c.lc.measure(ctx, frames, rows, **measure_kw)):
                        c.lcs[idx[j]] = ("detect", [item])
                except Exception as e:  # noqa: BLE001
                    for j in found:
                        c.lcs[idx[j]] = e
            if c.strip is not None:                   # the same frames, the same segments
                found = [j for j, r in enumerate(recs) if not int(r["status"]) and int(r["found"])]
                try:
                    rows = [(j, *c.strip.segs.detect_segment(_detection(recs[j], shape)[1], c.meas[idx[j]])) for j in found]
                    for j, item in zip(found, c.strip.measure(ctx, frames, rows, **measure_kw)):
                        c.strips[idx[j]] = ("detect", [item])
                except Exception as e:  # noqa: BLE001
                    for j in found:
                        c.strips[idx[j]] = e
            if c.radon is not None:                   # the frames without a detection, where the detect call left them
                todo = [j for j, r in enumerate(recs) if not int(r["status"]) and not int(r["found"])]
                try:
                    for j, line in c.radon.batch(ctx, frames, shape, todo, **measure_kw).items():
                        c.rlines[idx[j]] = line
                    for j, lc in c.radon.last_lc.items():
                        c.lcs[idx[j]] = lc if isinstance(lc, Exception) else ("radon", lc)
                    for j, st in c.radon.last_strip.items():
                        c.strips[idx[j]] = st if isinstance(st, Exception) else ("radon", st)
                except Exception as e:  # noqa: BLE001
                    for j in todo:
                        c.rlines[idx[j]] = e
                else:
                    if c.radon.null is not None:      # the same frames, while they are where the search read them
                        try:
                            from ..radon import null_seed
                            seeds = [null_seed(*c.keys[idx[j]]) for j in todo]
                            rl = {j: c.rlines[idx[j]] for j in todo}
                            for j, nulls in c.radon.null_batch(ctx, frames, shape, todo, seeds, rl, **measure_kw).items():
                                c.nulls[idx[j]] = nulls
                        except Exception as e:  # noqa: BLE001
                            for j in todo:
                                c.nulls[idx[j]] = e
            if c.streak is not None:                  # every frame of the chunk, where the detect call left it
                try:
                    for j, item in enumerate(c.streak.batch(ctx, frames, **measure_kw)):
                        c.streaks[idx[j]] = item
                except Exception as e:  # noqa: BLE001
                    for i in idx:
                        c.streaks[i] = e
            if c.sub is not None:                     # after every other measurement of the chunk: it changes the frames
                per_frame = {}
                try:
                    for j, r in enumerate(recs):
                        if int(r["status"]):
                            continue
                        found = int(r["found"])
                        per_frame[j] = _sub_segments(c, idx[j], found, _detection(r, shape)[1] if found else None, c.rlines[idx[j]])
                    for j, item in c.sub.run(ctx, frames, per_frame, **measure_kw).items():
                        c.subs[idx[j]] = item
                except Exception as e:  # noqa: BLE001
                    for j, (_, segs) in per_frame.items():
                        if segs:
                            c.subs[idx[j]] = e
        for i, rec in zip(idx, recs):
            c.rows[i] = rec
    except Exception as e:  # noqa: BLE001
        failed = e
    else:
        return
    for i in idx:                                     # (outside the handler: a frame's own exception is not chained to the call's)
        if second is None:
            c.rows[i] = failed
        else:
            _run_frame(c, i, filter, lambda: second(i))


def _emit(c, i, key, head, shape):
    """Frame i's text, from its slots: the sky row if it was normalised; the results row (``head``: its first 13 columns, or
    the header to take them from) or the errors entry; then the profiles row or the measurement's errors entry."""
    if c.srecs[i] is not None:
        c.sky.row(key, c.srecs[i])
    if c.strecs[i] is not None:
        c.stars.row(key, *c.strecs[i])
    if isinstance(c.seerecs[i], Exception):
        _log_error(c.errors, key, c.seerecs[i], c.debug)
    elif c.seerecs[i] is not None:
        c.seeing.row(key, *c.seerecs[i])
    try:
        row = c.rows[i]
        if isinstance(row, Exception):
            raise row
        detection, res, _ = row if isinstance(row, tuple) else _detection(row, shape)
        if detection:
            if not isinstance(head, str):
                head = " ".join(str(x) for x in (*key, *header_values(head, _HEADER_KEYS)))
            c.results.write(f"{head} {res['x1']} {res['y1']} {res['x2']} {res['y2']}\n")
    except Exception as e:  # noqa: BLE001
        _log_error(c.errors, key, e, c.debug)
        return
    if c.rounds is not None and c.trails[i] is not None:
        c.rounds.rows(key, *c.trails[i])
    if c.preview is not None and c.previews[i] is not None:
        try:
            if isinstance(c.previews[i], Exception):
                raise c.previews[i]
            c.preview.row(key, *c.previews[i], res if detection else None, c.trails[i] if detection else None)
        except Exception as e:  # noqa: BLE001 - a picture that cannot be made costs no other row
            _log_error(c.errors, key, e, c.debug)
    line = c.rlines[i]
    if isinstance(line, Exception):
        _log_error(c.errors, key, line, c.debug)
    elif line is not None:
        c.radon.row(key, line)
        if isinstance(c.nulls[i], Exception):
            _log_error(c.errors, key, c.nulls[i], c.debug)
        elif c.nulls[i] is not None:
            c.radon.null_rows(key, line, c.nulls[i])
    if isinstance(c.streaks[i], Exception):
        _log_error(c.errors, key, c.streaks[i], c.debug)
    elif c.streaks[i] is not None:
        c.streak.rows(key, *c.streaks[i])
    if c.masks is not None:                           # (after the rows above, which it does not touch)
        try:
            shp = c.shapes[i] or tuple(shape)           # (a frame that ran on its own may differ from the chunk's shape)
            if detection:
                c.masks.rows(key, shp, "detect", [c.masks.detect_segment(res, c.meas[i])])
            elif line is not None and not isinstance(line, Exception):
                c.masks.rows(key, shp, "radon", c.masks.radon_segments(line))
        except Exception as e:  # noqa: BLE001
            _log_error(c.errors, key, e, c.debug)
    if c.lc is not None and c.lcs[i] is not None:     # (after the rows it belongs to)
        if isinstance(c.lcs[i], Exception):
            _log_error(c.errors, key, c.lcs[i], c.debug)
        elif c.lcs[i][1]:
            c.lc.rows(key, *c.lcs[i])
    if c.strip is not None and c.strips[i] is not None:   # (after the frame's light-curve rows)
        if isinstance(c.strips[i], Exception):
            _log_error(c.errors, key, c.strips[i], c.debug)
        elif c.strips[i][1]:
            try:
                c.strip.rows(key, *c.strips[i])
            except Exception as e:  # noqa: BLE001 - a map that cannot be written costs no other row
                _log_error(c.errors, key, e, c.debug)
    if c.sub is not None and c.subs[i] is not None:   # (after the frame's strips rows)
        if isinstance(c.subs[i], Exception):
            _log_error(c.errors, key, c.subs[i], c.debug)
        else:
            try:
                c.sub.rows(key, *c.subs[i])
            except Exception as e:  # noqa: BLE001 - a frame that cannot be written costs no other row
                _log_error(c.errors, key, e, c.debug)
    if not detection or c.profiles is None:
        return
    try:                                              # (results.txt is written before, untouched)
        meas = c.meas[i] if c.meas[i] is not None else RuntimeError("no trail measurement")
        if isinstance(meas, Exception):
            raise meas
        c.profiles.add(key, *meas)
    except Exception as e:  # noqa: BLE001
        _log_error(c.errors, key, e, c.debug)


def process_field(results, errors, run, camcol, filter, field, params_bright, params_dim,
                  params_removestars, profiles=None, trail_params=None, sky=None, radon=None, stars=None, masks=None, lc=None,
                  strip=None, sub=None, seeing=None, rounds=None, preview=None, streak=None):
    """One frame end to end (reference: detecttrails.py:30-143): locate the frame (or its .bz2),
    read image + header + photoObj, detect, append ``run camcol filter field tai crpix1 crpix2
    crval1 crval2 cd11 cd12 cd21 cd22 x1 y1 x2 y2`` to ``results``; every exception is logged
    to ``errors`` (ids, 3-frame traceback, message) and swallowed.  ``profiles``: the sink (``add(key, trail, profile)``) the
    frame's trail profile goes to when it has a detection.  ``sky``: a ``_SkyStage``; the frame is normalised first and its
    sky.txt row written (detection and profile then refer to the normalised frame).  ``radon``: a ``_RadonStage``; a frame
    without a detection is searched for a faint trail and a line that is found gets its radon.txt row.  ``stars``: a
    ``_StarsStage``; the photoObj file is not opened, the catalogue is what the source finder finds in the frame (after the
    normalisation, if on), and the frame's stars.txt row is written.  ``masks``: a ``_MaskStage``; a results row, and every found
    faint line of ``radon`` with lines, gets its masks.txt row."""
    c = _Chunk(1, results, errors, params_bright, params_dim, params_removestars, profiles, trail_params, sky, radon, stars, masks, lc, strip, sub,
               seeing, rounds, preview, streak)
    c.keys[0] = (run, camcol, filter, field)
    head = None
    try:
        img, head, cat = _load_frame(run, camcol, filter, field, catalog=stars is None)
    except Exception as e:  # noqa: BLE001
        c.rows[0] = e
    else:
        _run_frame(c, 0, filter, lambda: (img, cat))
    _emit(c, 0, (run, camcol, filter, field), head, None)


def process_fields_batched(results, errors, ids, params_bright, params_dim, params_removestars, loaded=None, profiles=None,
                           trail_params=None):
    """Same outcome as calling process_field for every (run, camcol, filter, field) in ``ids``, in order -- the same
    results rows, the same errors entries, a bad frame costs only itself (detecttrails.py:119-139) -- but all frames
    that load go through ONE lfdmi_detect_batch call per (filter, shape) group.  ``loaded``: what ``_load_many(ids)``
    returned, if the caller read the files already."""
    from ..catalogs import pack_catalogs
    from .removestars import _check_finite
    if loaded is None:
        loaded = _load_many(ids)
    c = _Chunk(len(loaded), results, errors, params_bright, params_dim, params_removestars, profiles, trail_params, None)
    groups = {}
    for i, item in enumerate(loaded):
        if len(item) != 4:
            c.rows[i] = item[1]                       # did not load
            continue
        key, img, _, cat = item
        try:
            if cat is not None and len(cat["NOBSERVE"]):
                _check_finite(cat)                    # math.ceil(nan) in the reference: this frame's error alone
        except Exception as e:  # noqa: BLE001
            c.rows[i] = e
            continue
        groups.setdefault((key[2], img.shape), []).append(i)
    for (flt, shape), idx in groups.items():
        _run_group(c, idx, flt, shape, min(32, len(idx)),
                   lambda: (_np.stack([loaded[i][1] for i in idx]), pack_catalogs([loaded[i][3] for i in idx])),
                   lambda i: (loaded[i][1], loaded[i][3]))
    for i, item in enumerate(loaded):
        _emit(c, i, item[0], *((item[2], item[1].shape) if len(item) == 4 else (None, None)))


def process_loaded(results, errors, loaded, params_bright, params_dim, params_removestars, profiles=None, trail_params=None, sky=None,
                   radon=None, stars=None, masks=None, lc=None, strip=None, sub=None, seeing=None, rounds=None, preview=None,
                   streak=None):
    """process_fields_batched for a chunk the loader has read (``loader.Loaded``): the frames that sit in pinned memory go to
    the GPU as contiguous same-filter slices of that memory with the matching rows of the padded catalogue arrays (no copy
    of a frame on the host, no per-frame Python), the others take the per-frame path; rows and errors entries come out in
    the caller's order, each frame under its own try (detecttrails.py:119-139).  ``sky``: a
    ``_SkyStage``: every slice is normalised into the handle's device buffer first (the pinned big-endian slots go in as they
    are), detection and measurement run on that buffer, and one sky.txt row per normalised frame is written, in the caller's
    order, ahead of the frame's results row.  ``radon``: a ``_RadonStage``: after each slice's detection call its frames without
    a detection are searched where that call left them, and the lines found get their radon.txt rows.  ``stars``: a
    ``_StarsStage``: every slice's catalogue is built on the device from the frames the detect call is about to read (the
    loader's catalogue rows are not used), and one stars.txt row per frame is written after its sky row.  ``masks``: a
    ``_MaskStage``, as in ``process_field``.  ``rounds``: a ``_RoundsStage``: every slice's detect call is ``detect_rounds``."""
    import time
    t_in = time.perf_counter()
    n = len(loaded.keys)
    c = _Chunk(n, results, errors, params_bright, params_dim, params_removestars, profiles, trail_params, sky, radon, stars, masks, lc, strip, sub,
               seeing, rounds, preview, streak)
    c.keys = list(loaded.keys)
    by_slot = {}
    for i in range(n):
        if loaded.error[i] is not None:
            c.rows[i] = loaded.error[i]
        elif loaded.slot[i] >= 0:
            by_slot[loaded.slot[i]] = i
    # maximal runs of neighbouring slots with one filter
    slots = sorted(by_slot)
    runs, start = [], 0
    for j in range(1, len(slots) + 1):
        if j == len(slots) or slots[j] != slots[j - 1] + 1 or loaded.keys[by_slot[slots[j]]][2] != loaded.keys[by_slot[slots[start]]][2]:
            runs.append(slots[start:j])
            start = j
    shape = loaded.shape if getattr(loaded, "shape", None) else (loaded.buffer.shape[1:] if loaded.buffer is not None else (0, 0))
    if loaded.device is not None:                     # decompressed on the GPU and still there; swapped (and blotted) in place by
        frames_of, second, where = loaded.device.slice, None, ({}, {"native_device": True})      # the detect call: no second source
    else:
        frames_of, where = lambda a, b: loaded.buffer[a:b], ({"pinned": True}, {"pinned": True})
        second = lambda i: (loaded.buffer[loaded.slot[i]].astype(_np.float32), loaded.cat_of(i))  # noqa: E731
    for run_slots in runs:
        a, b = run_slots[0], run_slots[-1] + 1

        def source():
            cats = loaded.cats
            m = max(1, int(cats["count"][a:b].max()))
            packed = {k: _np.ascontiguousarray(v[a:b, :m]) for k, v in cats.items() if k != "count"}
            packed["count"] = cats["count"][a:b]
            return frames_of(a, b), packed
        idx = [by_slot[sl] for sl in run_slots]
        _run_group(c, idx, loaded.keys[idx[0]][2], shape, min(256, len(idx)), source, second, *where)
    for i in range(n):
        if c.rows[i] is None and loaded.array[i] is not None:    # not a plain float32 image of the chunk's shape, or an oversized catalogue
            _run_frame(c, i, loaded.keys[i][2], lambda: (loaded.array[i], loaded.cat_of(i)))
    for i, key in enumerate(loaded.keys):
        _emit(c, i, key, loaded.hdr[i], shape)
    if os.environ.get("LFD_LOADER_TRACE") == "1":
        print("[loader]   process_loaded: %.1f ms in all, %.1f ms inside lfdmi_detect_batch_raw" %
              (1e3 * (time.perf_counter() - t_in), 1e3 * c.gpu_s), flush=True)


class DetectTrails:
    """Process a selection of SDSS frames.

    ``DetectTrails(run=2888)``, ``DetectTrails(run=2888, camcol=1, filter='i')``,
    ``DetectTrails(run=2888, camcol=1, filter='i', field=139).process()`` ... at least one of
    run / camcol / filter / field (or frame) must be given.  ``results`` / ``errors`` /
    ``savepath`` choose the output files (appended to), ``debug`` switches all three parameter
    dictionaries to debug mode, ``params_bright`` / ``params_dim`` / ``params_removestars``
    replace the defaults; the dictionaries can also be edited on the instance afterwards.
    ``trail_profiles=True`` (default off) also measures the trail of every detected frame (``measure_trail``; include/lfdmi.h:
    trail profiles) and appends its ``profile_row`` to ``profiles`` (default ``<savepath>/profiles.txt``), one row per
    results.txt row, in the same order; ``trail_params`` (dict) replaces fields of lfdmi_trail_params.  Rank files, resume
    and ``Jobs`` merging treat profiles.txt as they treat results.txt.
    ``defocus=True`` (default off; implies ``trail_profiles``) also fits every profiles row against the defocus bank
    (``lfd_amd.defocus``; include/lfdmi.h: defocus fit) and writes one row per results.txt row to ``defocus_file`` (default
    ``<savepath>/defocus.txt``): ``run camcol filter field status h_km h_lo h_hi radius_m seeing_arcsec shift amplitude offset
    chi2 dof chi2_focus model_ofwhm model_depth``.  ``defocus_params`` (dict): heights, radii, seeings, instrument, ovs,
    max_shift, delta_chi2.  The bank is built once per process; rank files, resume and ``Jobs`` treat defocus.txt like
    profiles.txt.
    ``normalize=True`` (default off): every frame goes through the sky normalisation first (include/lfdmi.h: sky normalisation;
    ``sky_params``: dict or ``lfd_amd.sky.SkyParams``) -- for frames that still carry their sky (fpC files, raw exposures).  The
    loader's big-endian pinned slots are normalised into a device buffer and detected there.  ``sky_file`` (default
    ``<savepath>/sky.txt``) gets one row per frame that loaded: ``run camcol filter field status sky sigma gain n_empty``,
    written ahead of the chunk's progress marks; rank files, resume and ``Jobs`` treat it like results.txt.  Profiles and
    defocus fits then refer to the normalised frame: flux = value / gain + sky.
    ``find_stars=True`` (default off): for frames that have no photoObj table.  The loader does not open photoObj files; each
    chunk's remove_stars catalogue is what the source finder finds in its frames (include/lfdmi.h: source finder;
    ``stars_params``: dict or ``lfd_amd.stars.StarsParams``), after the normalisation when that is on (sigma ``target_sigma``,
    otherwise 0.025).  ``stars_file`` (default ``<savepath>/stars.txt``) gets one row per frame that loaded: ``run camcol
    filter field status n_found n_out n_extended``; rank files, resume and ``Jobs`` treat it like sky.txt.  Every other output of
    a run without ``find_stars`` stays byte for byte what it is.
    ``seeing=True`` (default off): every chunk's stars are measured before detection blots them (include/lfdmi.h: frame
    seeing; ``seeing_params``: dict or ``lfd_amd.psf.PsfParams``), on the finder's device records with ``find_stars=True`` and
    on a finder run of its own (``stars_params``) otherwise.  ``seeing_file`` (default ``<savepath>/seeing.txt``) gets one row
    per frame that loaded: ``run camcol filter field status n_cand n_ok n_used fwhm_px fwhm_arcsec seeing_arcsec scatter
    ell``.  With ``defocus=True`` every fit behind defocus.txt and radon_defocus.txt gets its frame's ``seeing_arcsec`` as
    ``fit_defocus``'s ``seeing`` (NaN, a free fit, for a frame with too few stars).  Rank files, resume and ``Jobs`` treat
    seeing.txt like stars.txt; a run without ``seeing`` stays byte for byte what it is.
    ``streaks=True`` (default False: nothing differs and no file appears): every chunk is searched for short streaks after its
    detect call, while its frames are on the device and blotted by remove_stars (include/lfdmi.h: short-streak search;
    ``streaks_params``: dict of bin, length, max_streaks, peel_halfwidth, clip, threshold, checked here), and ``streaks_file``
    (default ``<savepath>/streaks.txt``) gets one row per found streak: ``run camcol filter field streak q s r0 c0 n_pix snr x1 y1
    x2 y2``.  Rank files, resume and ``Jobs`` treat streaks.txt like previews.txt.

    ``previews="detections"`` or ``"all"`` (default None: nothing differs and no file appears): every chunk is turned into small
    8-bit images on the device (include/lfdmi.h: frame previews; ``preview_params``: dict of bin, mode, lo_ppm, hi_ppm, limits,
    kind, softening, lut, color, thick) before detection blots it, after the normalisation when that is on.  The images of the
    frames that get a results.txt row (``"detections"``), or of every frame that loaded (``"all"``), are copied back, overlaid
    with the row's line (and the trails.txt lines with ``max_trails``; ``lfd_amd.previews.overlay``) and written to
    ``preview_dir`` (default ``<savepath>/previews``) as ``frame-{filter}-{run:06d}-{camcol}-{field:04}.fits.png``, the name the
    reference's image checker looks for.  ``previews_file`` (default ``<savepath>/previews.txt``) gets one row per picture: ``run
    camcol filter field status bin lo hi n_cells n_empty file``.  Rank files, resume and ``Jobs`` treat previews.txt like
    seeing.txt; the pictures' names are unique per frame and carry no rank suffix.  Every other output stays byte for byte what
    it is.
    ``radon=True`` (default off): after each chunk's detection call the frames WITHOUT a detection are searched for a trail that
    is faint in every pixel but long (include/lfdmi.h: faint-trail search; ``radon_params``: dict or
    ``lfd_amd.radon.RadonParams``), with the sky sigma ``target_sigma`` under ``normalize=True`` and 0.025 otherwise.  A line
    that is found gets a row in ``radon_file`` (default ``<savepath>/radon.txt``): ``run camcol filter field x1 y1 x2 y2 snr
    n_pix``.  results.txt does not change with it.  ``radon_lines=K`` (default None: one line per frame, as above): up to K
    lines per frame by peeling (steps 7 - 9 of the definition; ``radon_lines_params``: dict or ``lfd_amd.radon.RadonLinesParams``
    with ``peel_halfwidth`` and ``min_seg``).  radon.txt then gets one row per found line, in peel order, and
    ``radon_segments_file`` (default ``<savepath>/radon_segments.txt``) one row per found line with where the trail starts and
    stops: ``run camcol filter field line ex1 ey1 ex2 ey2 seg_snr seg_n_pix``; rank files and resume treat it like radon.txt.
    ``radon_profiles=True`` (needs ``radon_lines``): every found line's segment is measured by the stacked cross-sections
    (include/lfdmi.h: stacked cross-sections; ``stack_params``: dict or ``lfd_amd.stack.StackParams``) on the frames where the
    search left them, and ``radon_profiles_file`` (default ``<savepath>/radon_profiles.txt``) gets one row per found line: ``run
    camcol filter field line status x1 y1 x2 y2 n_col background noise peak fwhm fwhm_arcsec depth flux flux_err snr``.  With
    ``defocus=True`` the rows are fitted too (a bank built for the stack's prof_half / step / wing) and written to
    ``radon_defocus_file`` (default ``<savepath>/radon_defocus.txt``): defocus.txt's columns with the line's index after the
    field.  Rank files and resume treat both like radon_segments.txt; every other output stays byte for byte what it is.
    ``radon_short=True`` or a dict / ``lfd_amd.radon.RadonShortParams`` (needs ``radon=True``): the frames are also searched
    for short faint trails on every dyadic level (steps 10 - 12 of the definition) and ``radon_short_file`` (default
    ``<savepath>/radon_short.txt``) gets one row per found candidate: ``run camcol filter field line level strip snr n_pix ex1
    ey1 ex2 ey2 seg_snr seg_n_pix``; radon.txt and radon_segments.txt stay what they are without it.  With
    ``radon_profiles=True`` (then ``radon_lines`` may be None) the short segments are measured too, and every row of
    radon_profiles.txt ends with its source, ``lines`` or ``short``.
    ``radon_null=K`` (1 .. 64; needs ``radon=True``): every searched frame also gets its null peaks (include/lfdmi.h: null
    peaks, steps 17 - 20) of each kind that is on -- lines, and short / wide where ``radon_short`` / ``radon_wide`` are -- while the
    chunk's frames are on the device, seeded by ``lfd_amd.radon.null_seed(run, camcol, filter, field)``, so resume and any rank
    split give the same rows.  ``radon_null_file`` (default ``<savepath>/radon_null.txt``) gets one row per frame and kind: ``run
    camcol filter field kind K null_min null_median null_max``; ``radon_fap_file`` (``<savepath>/radon_fap.txt``) one row per found
    line: ``run camcol filter field kind line snr n_ge K fap``.  Rank files and resume treat both like radon.txt; every other
    output stays byte for byte what it is.  ``radon_null_scheme`` ("scramble", the default; "signflip", "rowshift", "colshift":
    include/lfdmi.h steps 21 - 22) fills both files with that scheme's peaks, in the same columns.
    ``radon_null_rounds=True`` (needs ``radon_null_scheme="signflip"``): every peel round k >= 1 that a frame's search of a kind
    ran also gets its own null, the frame with that search's lines 0 .. k-1 blotted as the search blotted them;
    ``radon_null_rounds_file`` (default ``<savepath>/radon_null_rounds.txt``) gets one row per frame, kind and such round: ``run
    camcol filter field kind round K null_min null_median null_max``, and the radon_fap.txt row of line k >= 1 is taken from
    round k's peaks, not round 0's.  Rank files and resume treat the file like radon_null.txt.
    ``radon_wide=True`` or a dict / ``lfd_amd.radon.RadonWideParams`` (needs ``radon=True``): the frames are also searched for
    wide faint trails by scoring sliding bands of the last level's lines (steps 13 - 16 of the definition) and
    ``radon_wide_file`` (default ``<savepath>/radon_wide.txt``) gets one row per found band: ``run camcol filter field line
    width width_px snr n_pix ex1 ey1 ex2 ey2 seg_snr seg_n_pix``; rank files and resume treat it like radon_short.txt and
    every other output stays what it is without it.  With ``radon_lines=None`` and no ``radon_short`` the wide call's plain
    records are the frame's one line, which saves a transform.  With ``radon_profiles=True`` the bands' segments are measured
    too and their rows end with ``wide``.
    ``trail_masks=True`` (default off): every results.txt row gets one row in ``masks_file`` (default ``<savepath>/masks.txt``),
    in the same order: ``run camcol filter field source line x1 y1 x2 y2 half n_pix`` with source ``detect`` -- the band of
    half-width ``half`` around the segment, flagged by ``lfdmi_mask_trails`` (include/lfdmi.h: trail masks; cap 0), and the
    number of the frame's pixels in it.  With ``trail_profiles=True`` the segment is the trail's refined extent and ``half``
    comes from its fwhm (``lfd_amd.masks.half_width``; ``mask_params``: dict of its keywords k_fwhm, min_half, grow,
    default_half); without a measurement it is the results row's line and the default half-width.  With ``radon_lines=K`` every
    found faint line also gets a row, source ``radon``, its segment ex1 .. ey2, ``half`` from ``radon_profiles``' fwhm when that
    is on.  ``mask_dir``: each masked frame's plane is written there as ``mask-<run>-<camcol>-<filter>-<field>.npz`` (``bits``,
    ``shape``: ``masks.pack``).  Rank files, resume and ``Jobs`` treat masks.txt like profiles.txt; every other output stays
    byte for byte what it is.
    ``light_curves=True`` (default off): every results.txt row and, with ``radon_lines=K``, every found faint line is measured in
    sections along its segment (include/lfdmi.h: light curves; ``lc_params``: dict of lfdmi_lc_params fields) -- the segment and
    half-width of ``trail_masks`` (``mask_params``), the sky bands of ``lfd_amd.lightcurve.segments`` -- where its frame is still
    on the device.  ``lightcurves_file`` (default ``<savepath>/lightcurves.txt``) gets one row per section that is not EMPTY:
    ``run camcol filter field source line section t0 t1 n_geom n_core n_sky bkg flux flux_err rate rate_err status``;
    ``lightcurve_summary_file`` (default ``<savepath>/lightcurve_summary.txt``) one row per segment: ``run camcol filter field
    source line status n_sec n_ok mean_rate mean_rate_err chi2 dof peak_section peak_rate length flux flux_err``.  The default
    ``clip`` (0.125) is the faint-trail units' star cut; a bright trail needs ``lc_params={"clip": ...}`` above its peak.  Rank files,
    resume and ``Jobs`` treat both like masks.txt; every other output stays byte for byte what it is.

    ``max_trails=K`` (1 .. 8; unset or 1: nothing differs and no file appears): the chunk pipeline calls ``detect_rounds`` where it
    called detect (include/lfdmi.h: detection rounds; ``rounds_params``: dict of half, dup_dist) and uses record 0 for everything
    it did before, so results.txt and every other output stay byte for byte what they are; ``trails_file`` (default
    ``<savepath>/trails.txt``) gets one row per found trail, round 0 included: ``run camcol filter field round found rho theta x1
    y1 x2 y2 dup_of`` (``lfd_amd.rounds.read_trails``).  Rank files, resume and ``Jobs`` treat it like masks.txt.  The extra
    trails are not fed to the other stages.
    ``trail_strips=True`` (default off): the same segments, at the same places, are straightened into maps of sections along the
    trail by offsets across it (include/lfdmi.h: trail strips; ``strips_params``: dict of lfdmi_strip_params fields), each
    half-width widened by ``wing`` so that the wings are sky.  ``strips_file`` (default ``<savepath>/strips.txt``) gets one row
    per section that is not EMPTY: ``run camcol filter field source line section t0 t1 n_core n_wing bkg rate rate_err centre
    width status``.  ``strips_dir``: each segment's maps are written there as ``strip-<run>-<camcol>-<filter>-<field>-<source>
    <line>.npz`` (``mean``, ``n``, ``n_geom``, ``segment`` = x1 y1 x2 y2 half) with a ``.png`` preview beside it.  Rank files,
    resume and ``Jobs`` treat strips.txt like lightcurves.txt; every other output stays byte for byte what it is.
    ``subtract_trails=True`` (default off): the same segments, each half-width widened by ``wing``, are modelled from their own
    strips and taken out of the frames (include/lfdmi.h: trail subtraction; ``sub_params``: dict of lfdmi_sub_params fields),
    after every other measurement of the chunk, because it changes the frames, and while they are still on the device.
    ``subtracted_file`` (default ``<savepath>/subtracted.txt``) gets one row per segment: ``run camcol filter field source line
    status n_sec n_usable n_model n_pix removed peak peak_section``.  ``clean_dir``: each changed frame is written there as
    ``clean-<run>-<camcol>-<filter>-<field>.npz`` (float32 ``frame`` in buffer order, and its ``segments``).  Rank files, resume
    and ``Jobs`` treat subtracted.txt like strips.txt; every other output stays byte for byte what it is.
    """

    _FILTERS = ('u', 'g', 'r', 'i', 'z')
    _CAMCOLS = (1, 2, 3, 4, 5, 6)

    def __init__(self, **kwargs):
        save = kwargs.get("savepath", ".")
        self.kwargs = kwargs
        self.params_bright, self.params_dim, self.params_removestars = default_params()
        self.results = kwargs.get("results", os.path.join(save, "results.txt"))
        self.errors = kwargs.get("errors", os.path.join(save, "errors.txt"))
        self.defocus = bool(kwargs.get("defocus", False))
        self.defocus_file = kwargs.get("defocus_file", os.path.join(save, "defocus.txt"))
        self.defocus_params = dict(kwargs.get("defocus_params") or {})
        self.trail_profiles = bool(kwargs.get("trail_profiles", False)) or self.defocus
        self.profiles = kwargs.get("profiles", os.path.join(save, "profiles.txt"))
        self.trail_params = dict(kwargs.get("trail_params") or {})
        self.normalize = bool(kwargs.get("normalize", False))
        self.sky_file = kwargs.get("sky_file", os.path.join(save, "sky.txt"))
        from ..sky import as_params
        self.sky_params = as_params(kwargs.get("sky_params"))
        if self.normalize:
            _native.make_sky_params(**self.sky_params)          # (unknown names raise here, not per frame)
        self.find_stars = bool(kwargs.get("find_stars", False))
        self.stars_file = kwargs.get("stars_file", os.path.join(save, "stars.txt"))
        from ..stars import as_params as stars_as_params
        self.stars_params = stars_as_params(kwargs.get("stars_params"))    # (out-of-range values raise here, not per frame)
        self.seeing = bool(kwargs.get("seeing", False))
        self.seeing_file = kwargs.get("seeing_file", os.path.join(save, "seeing.txt"))
        from ..psf import as_params as psf_as_params
        self.seeing_params = psf_as_params(kwargs.get("seeing_params"))  # (likewise)
        self.streaks = bool(kwargs.get("streaks", False))
        self.streaks_file = kwargs.get("streaks_file", os.path.join(save, "streaks.txt"))
        from ..streaks import as_params as streak_as_params
        self.streaks_params = streak_as_params(kwargs.get("streaks_params"))   # (a bad value stops here, not in the first chunk)
        self.previews = kwargs.get("previews")
        if self.previews not in (None, "detections", "all"):
            raise ValueError("previews must be None, 'detections' or 'all'")
        self.preview_dir = kwargs.get("preview_dir", os.path.join(save, "previews"))
        self.previews_file = kwargs.get("previews_file", os.path.join(save, "previews.txt"))
        from ..previews import as_params as preview_as_params
        self.preview_params = preview_as_params(kwargs.get("preview_params"))   # (likewise)
        self.radon = bool(kwargs.get("radon", False))
        self.radon_file = kwargs.get("radon_file", os.path.join(save, "radon.txt"))
        from ..radon import as_params as radon_as_params
        self.radon_params = radon_as_params(kwargs.get("radon_params"))
        self.radon_lines = kwargs.get("radon_lines")
        self.radon_segments_file = kwargs.get("radon_segments_file", os.path.join(save, "radon_segments.txt"))
        self.radon_lines_params = {}
        if self.radon_lines is not None:
            from ..radon import RadonLinesParams, RadonParams, as_lines_params
            lp = {k: v for k, v in as_lines_params(kwargs.get("radon_lines_params")).items() if k != "max_lines"}
            RadonLinesParams(**dict(lp, max_lines=self.radon_lines)).validate(RadonParams(**self.radon_params).min_len)
            self.radon_lines_params = lp
        self.radon_profiles = bool(kwargs.get("radon_profiles", False))
        self.radon_profiles_file = kwargs.get("radon_profiles_file", os.path.join(save, "radon_profiles.txt"))
        self.radon_defocus_file = kwargs.get("radon_defocus_file", os.path.join(save, "radon_defocus.txt"))
        self.radon_short_file = kwargs.get("radon_short_file", os.path.join(save, "radon_short.txt"))
        self.radon_short = None
        rs = kwargs.get("radon_short", False)
        if rs is not False and rs is not None:
            if not self.radon:
                raise ValueError("radon_short needs radon=True: it is a mode of the faint-trail search")
            from ..radon import RadonParams, as_short_params
            self.radon_short = as_short_params(None if rs is True else rs, RadonParams(**self.radon_params).bin)
        self.radon_wide_file = kwargs.get("radon_wide_file", os.path.join(save, "radon_wide.txt"))
        self.radon_wide = None
        rw = kwargs.get("radon_wide", False)
        if rw is not False and rw is not None:
            if not self.radon:
                raise ValueError("radon_wide needs radon=True: it is a mode of the faint-trail search")
            from ..radon import RadonParams, as_wide_params
            self.radon_wide = as_wide_params(None if rw is True else rw, RadonParams(**self.radon_params).min_len)
        self.stack_params = {}
        self.radon_null_file = kwargs.get("radon_null_file", os.path.join(save, "radon_null.txt"))
        self.radon_fap_file = kwargs.get("radon_fap_file", os.path.join(save, "radon_fap.txt"))
        self.radon_null = kwargs.get("radon_null")
        if self.radon_null is not None:
            if not self.radon:
                raise ValueError("radon_null needs radon=True: it is a measurement of the faint-trail search")
            if int(self.radon_null) != self.radon_null or not 1 <= self.radon_null <= _native.RADON_NULL_MAX:
                raise ValueError("radon_null must be an integer, 1 .. %d" % _native.RADON_NULL_MAX)
            self.radon_null = int(self.radon_null)
        self.radon_null_rounds_file = kwargs.get("radon_null_rounds_file", os.path.join(save, "radon_null_rounds.txt"))
        self.radon_null_scheme = kwargs.get("radon_null_scheme", "scramble")
        self.radon_null_rounds = kwargs.get("radon_null_rounds", False)
        if self.radon_null_scheme not in _native.RADON_NULL_SCHEMES:
            raise ValueError("radon_null_scheme must be one of %s" % ", ".join(_native.RADON_NULL_SCHEMES))
        if self.radon_null_rounds not in (True, False):
            raise ValueError("radon_null_rounds must be True or False")
        if (self.radon_null_scheme != "scramble" or self.radon_null_rounds) and self.radon_null is None:
            raise ValueError("radon_null_scheme and radon_null_rounds need radon_null=K")
        if self.radon_null_rounds and self.radon_null_scheme != "signflip":
            raise ValueError("radon_null_rounds needs radon_null_scheme='signflip': the other schemes move the pixels from under a "
                             "peeled line's band")
        if self.radon_profiles:
            if not self.radon or (self.radon_lines is None and self.radon_short is None and self.radon_wide is None):
                raise ValueError("radon_profiles=True needs radon=True and radon_lines=K: the segments it measures are theirs")
            from ..stack import as_params as stack_as_params
            self.stack_params = stack_as_params(kwargs.get("stack_params"))
        self.trails_file = kwargs.get("trails_file", os.path.join(save, "trails.txt"))
        self.max_trails = kwargs.get("max_trails")
        self.rounds_params = None
        if self.max_trails is not None:
            from ..rounds import MAX_TRAILS, as_params as rounds_as_params
            if int(self.max_trails) != self.max_trails or not 1 <= self.max_trails <= MAX_TRAILS:
                raise ValueError("max_trails must be an integer, 1 .. %d" % MAX_TRAILS)
            self.max_trails = int(self.max_trails)
            self.rounds_params = rounds_as_params(kwargs.get("rounds_params"), max_trails=self.max_trails)
            _native.make_rounds_params(**self.rounds_params)     # (bad values raise here, not per frame)
        elif kwargs.get("rounds_params") is not None:
            raise ValueError("rounds_params needs max_trails=K")
        self.rounds = self.max_trails is not None and self.max_trails > 1
        self.trail_masks = bool(kwargs.get("trail_masks", False))
        self.masks_file = kwargs.get("masks_file", os.path.join(save, "masks.txt"))
        self.mask_dir = kwargs.get("mask_dir")
        self.mask_params = dict(kwargs.get("mask_params") or {})
        if self.trail_masks:
            from ..masks import half_width
            half_width(1.0, **self.mask_params)                  # (unknown names raise here, not per frame)
        self.light_curves = bool(kwargs.get("light_curves", False))
        self.lightcurves_file = kwargs.get("lightcurves_file", os.path.join(save, "lightcurves.txt"))
        self.lightcurve_summary_file = kwargs.get("lightcurve_summary_file", os.path.join(save, "lightcurve_summary.txt"))
        self.lc_params = dict(kwargs.get("lc_params") or {})
        if self.light_curves:
            from ..lightcurve import as_params as lc_as_params
            from ..masks import half_width
            lc_as_params(self.lc_params)                         # (unknown names and bad values raise here, not per frame)
            half_width(1.0, **self.mask_params)
        self.trail_strips = bool(kwargs.get("trail_strips", False))
        self.strips_file = kwargs.get("strips_file", os.path.join(save, "strips.txt"))
        self.strips_dir = kwargs.get("strips_dir")
        self.strips_params = dict(kwargs.get("strips_params") or {})
        if self.trail_strips:
            from ..masks import half_width
            from ..strips import as_params as strips_as_params
            strips_as_params(self.strips_params)                 # (unknown names and bad values raise here, not per frame)
            half_width(1.0, **self.mask_params)
        self.subtract_trails = bool(kwargs.get("subtract_trails", False))
        self.subtracted_file = kwargs.get("subtracted_file", os.path.join(save, "subtracted.txt"))
        self.clean_dir = kwargs.get("clean_dir")
        self.sub_params = dict(kwargs.get("sub_params") or {})
        if self.subtract_trails:
            from ..masks import half_width
            _SubStage(None, self.sub_params)                     # (unknown names and bad values raise here, not per frame)
            half_width(1.0, **self.mask_params)
        if self.trail_profiles:
            _native.make_trail_params(**self.trail_params)      # (unknown names raise here, not per frame)
        if self.defocus:
            from .. import defocus
            defocus.make_params(**self.defocus_params, **self.trail_params)   # (likewise)
        for name in ("params_bright", "params_dim", "params_removestars"):
            if name in kwargs:
                setattr(self, name, kwargs[name])
        if "debug" in kwargs:
            self.debug = kwargs.pop("debug")
            for d in (self.params_bright, self.params_dim, self.params_removestars):
                d["debug"] = self.debug
        if any(d["debug"] for d in (self.params_removestars, self.params_bright, self.params_dim)):
            setup_debug()
        self._load()

    def _runInfo(self):
        rl = sdssfiles.runlist()
        w = _np.nonzero(rl["run"] == self._run)[0]
        if len(w) == 0:
            raise ValueError("Run %s not found in runList.par" % self._run)
        return int(rl["startfield"][w[0]]), int(rl["endfield"][w[0]])

    def _getRuns(self):
        return [int(r) for r in sdssfiles.runlist()["run"]]

    def _load(self):
        """Selection mode from the keywords given (detecttrails.py:290-342): run, run-camcol,
        run-filter, run-camcol-filter, camcol-filter, camcol-frame, field."""
        kw = self.kwargs
        self._run = self._camcol = self._field = 0
        self._filter = self._pick = "0"
        if "run" in kw:
            self._run, self._pick = kw["run"], "run"
        if "camcol" in kw:
            if kw["camcol"] not in self._CAMCOLS:
                raise ValueError("Nonexisting camcol")
            self._camcol, self._pick = kw["camcol"], "run-camcol"
        if "field" in kw or "frame" in kw:
            if self._camcol == 0:
                raise ValueError("send camcol= ")
            self._field = kw["field"] if "field" in kw else kw["frame"]
        if "filter" in kw:
            if kw["filter"] not in self._FILTERS:
                raise ValueError("Nonexistting filter")
            self._filter = kw["filter"]
            if self._camcol != 0:
                self._pick = "camcol-filter"
            if self._run != 0:
                self._pick = "run-filter"
            if self._camcol != 0 and self._run != 0:
                self._pick = "run-camcol-filter"
        elif self._field != 0 and self._camcol != 0:
            self._pick = "camcol-frame"
        if self._field != 0 and self._camcol != 0 and self._filter != "0":
            self._pick = "field"

    def _frames(self):
        """Yield (run, camcol, filter, field) in the reference's loop order (detecttrails.py:350-407)."""
        pick = self._pick
        if pick == "camcol-filter":
            for run in self._getRuns():
                self._run = run
                start, end = self._runInfo()
                for field in range(start, end):
                    yield run, self._camcol, self._filter, field
            self._run = 0
        elif pick == "run":
            start, end = self._runInfo()
            for camcol in self._CAMCOLS:
                for flt in self._FILTERS:
                    for field in range(start, end):
                        yield self._run, camcol, flt, field
        elif pick == "run-filter":
            start, end = self._runInfo()
            for camcol in self._CAMCOLS:
                for field in range(start, end):
                    yield self._run, camcol, self._filter, field
        elif pick == "run-camcol":
            start, end = self._runInfo()
            for flt in self._FILTERS:
                for field in range(start, end, 50):  # the reference samples every 50th field here
                    yield self._run, self._camcol, flt, field
        elif pick == "run-camcol-filter":
            start, end = self._runInfo()
            for field in range(start, end):
                yield self._run, self._camcol, self._filter, field
        elif pick == "camcol-frame":
            for flt in self._FILTERS:
                yield self._run, self._camcol, flt, self._field
        elif pick == "field":
            yield self._run, self._camcol, self._filter, self._field

    def process(self, batch=32, rank=None, world_size=None, loader_threads=None, resume=False):
        """Run the selection; results and errors files are opened in append mode.

        At most ``batch`` frames go to the GPU per call (same rows, same order as frame by frame; ``batch=1`` is the
        reference's frame-at-a-time loop).  A pool of ``loader_threads`` reader threads (default: one per core, at most 32;
        $LFD_LOADER_THREADS) reads the FITS / .fits.bz2 files of the next chunk straight into page-locked staging memory
        while the GPU works on the current one (``loader.FrameLoader``; chunks of min(batch, $LFD_LOADER_SLOTS = 64, or 256 for a selection of .fits.bz2 files) frames:
        two 0.8 GB staging buffers keep the link busy, larger ones only cost set-up time); the big-endian floats are swapped
        on the device.  With ``world_size`` > 1 (default: $RANK / $WORLD_SIZE, i.e. one process per GPU under torchrun) every
        rank processes one contiguous block of the selection (``lfd_amd.batch.shard_bounds``: ceil(n / world_size) frames
        each, the same rule the batch detector and bench.py use) and appends to ``<results>.rank<r>`` / ``<errors>.rank<r>``
        -- the replacement for splitting runs into PBS jobs (lfd/createjobs/createjobs.py:173-202).

        ``resume=True``: frames listed in ``<results>[.rank<r>].progress`` (appended to, chunk by chunk, after the chunk's rows
        and error entries have been flushed) are skipped, so a run that was interrupted continues where it stopped instead
        of appending its rows twice (the reference restarts a PBS job from its first frame).

        ``self.last_stats`` afterwards: frames, total seconds, set-up seconds (context + staging buffers) and the seconds
        after which every chunk was done."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        from ..batch import shard_range
        from .loader import FrameLoader
        t_start = time.perf_counter()
        rank = int(os.environ.get("RANK", 0)) if rank is None else rank
        world_size = int(os.environ.get("WORLD_SIZE", 1)) if world_size is None else world_size
        suffix = f".rank{rank}" if world_size > 1 else ""
        keys = list(self._frames())
        n_selection = len(keys)
        if world_size > 1:
            a, b = shard_range(len(keys), rank, world_size)
            keys = keys[a:b]
        progress_path = self.results + suffix + ".progress"
        # first line of the progress file: what the marks below it belong to.  A resume only trusts marks written for the same
        # selection, shard and world size; anything else (an older run of another selection into the same savepath, a change
        # of world_size: the marks would be compared against a different shard) is refused, not silently applied.
        header = "# lfd-progress v1 pick=%s run=%s camcol=%s filter=%s field=%s rank=%d world_size=%d selection=%d" % (
            self._pick, self.kwargs.get("run", 0), self._camcol, self._filter, self._field, rank, world_size, n_selection)
        skipped = 0
        fresh = True
        if resume and os.path.exists(progress_path):
            with open(progress_path) as f:
                lines = [ln.strip() for ln in f if ln.strip()]
            if lines:
                if lines[0] != header:
                    raise ValueError("resume=True: %s was written for another selection / shard (%r, this run: %r); "
                                     "delete it or run with resume=False" % (progress_path, lines[0], header))
                done = {tuple(ln.split()) for ln in lines[1:]}
                before = len(keys)
                keys = [k for k in keys if tuple(str(x) for x in k) not in done]
                skipped = before - len(keys)
                fresh = False
        self.last_stats = {"frames": len(keys), "chunk_frames": 0, "setup_s": 0.0, "chunk_done_s": [], "seconds": 0.0,
                           "skipped_by_resume": skipped}
        # resume=False starts a new record of marks (an earlier run's marks must never make a later resume skip frames this
        # run did not process); rows and errors are appended to, as in the reference
        import contextlib
        with open(self.results + suffix, "a") as results, open(self.errors + suffix, "a") as errors, \
                open(progress_path, "w" if fresh else "a") as progress, \
                (open(self.profiles + suffix, "a") if self.trail_profiles else contextlib.nullcontext()) as profiles, \
                (open(self.defocus_file + suffix, "a") if self.defocus else contextlib.nullcontext()) as defocus_out, \
                (open(self.sky_file + suffix, "a") if self.normalize else contextlib.nullcontext()) as sky_out, \
                _both(open(self.stars_file + suffix, "a") if self.find_stars else contextlib.nullcontext(),
                      open(self.seeing_file + suffix, "a") if self.seeing else contextlib.nullcontext()) as (stars_out, seeing_out), \
                (open(self.radon_file + suffix, "a") if self.radon else contextlib.nullcontext()) as radon_out, \
                (open(self.radon_segments_file + suffix, "a") if self.radon and self.radon_lines is not None
                 else contextlib.nullcontext()) as segments_out, \
                (open(self.radon_short_file + suffix, "a") if self.radon_short is not None else contextlib.nullcontext()) as short_out, \
                (open(self.radon_wide_file + suffix, "a") if self.radon_wide is not None else contextlib.nullcontext()) as wide_out, \
                _both(open(self.radon_profiles_file + suffix, "a") if self.radon_profiles else contextlib.nullcontext(),
                      _both(open(self.radon_null_file + suffix, "a") if self.radon_null is not None else contextlib.nullcontext(),
                            _both(open(self.radon_fap_file + suffix, "a") if self.radon_null is not None
                                  else contextlib.nullcontext(),
                                  open(self.radon_null_rounds_file + suffix, "a") if self.radon_null_rounds
                                  else contextlib.nullcontext()))) as (rprof_out, (null_out, (fap_out, rounds_out))), \
                (open(self.radon_defocus_file + suffix, "a") if self.radon_profiles and self.defocus
                 else contextlib.nullcontext()) as rdef_out, \
                _both(open(self.masks_file + suffix, "a") if self.trail_masks else contextlib.nullcontext(),
                      open(self.trails_file + suffix, "a") if self.rounds else contextlib.nullcontext()) as (masks_out, trails_out), \
                (open(self.lightcurves_file + suffix, "a") if self.light_curves else contextlib.nullcontext()) as lc_out, \
                (open(self.lightcurve_summary_file + suffix, "a") if self.light_curves else contextlib.nullcontext()) as lcsum_out, \
                _both(open(self.strips_file + suffix, "a") if self.trail_strips else contextlib.nullcontext(),
                      _both(open(self.subtracted_file + suffix, "a") if self.subtract_trails else contextlib.nullcontext(),
                            _both(open(self.previews_file + suffix, "a") if self.previews is not None
                                  else contextlib.nullcontext(),
                                  open(self.streaks_file + suffix, "a") if self.streaks
                                  else contextlib.nullcontext()))) as (strips_out, (sub_out, (previews_out, streaks_out))):
            seeing = None
            if self.seeing:
                sigma = _native.make_sky_params(**self.sky_params).target_sigma if self.normalize else 0.025
                grid = self.defocus_params.get("seeings")
                if grid is None:
                    from ..defocus import default_params as defocus_defaults
                    grid = defocus_defaults()["seeings"]
                seeing = _SeeingStage(seeing_out, self.seeing_params, sigma, self.stars_params, self.params_removestars["pixscale"], grid)
            if self.trail_profiles:
                profiles = _DefocusTee(profiles, defocus_out, self.defocus_params, self.trail_params, seeing)
            prof_kw = {"profiles": profiles, "trail_params": self.trail_params} if self.trail_profiles else {}
            sky = _SkyStage(sky_out, self.sky_params) if self.normalize else None
            if sky is not None:
                prof_kw["sky"] = sky
            stars = None
            if self.find_stars:
                sigma = _native.make_sky_params(**self.sky_params).target_sigma if self.normalize else 0.025
                stars = prof_kw["stars"] = _StarsStage(stars_out, self.stars_params, sigma)
            lc = None
            if self.light_curves:
                sigma = _native.make_sky_params(**self.sky_params).target_sigma if self.normalize else 0.025
                lc = prof_kw["lc"] = _LcStage(lc_out, lcsum_out, self.lc_params, sigma, self.mask_params)
            strip = None
            if self.trail_strips:
                sigma = _native.make_sky_params(**self.sky_params).target_sigma if self.normalize else 0.025
                strip = prof_kw["strip"] = _StripStage(strips_out, self.strips_params, sigma, self.mask_params, self.strips_dir)
            radon = None
            if self.radon:
                sigma = _native.make_sky_params(**self.sky_params).target_sigma if self.normalize else 0.025
                radon = prof_kw["radon"] = _RadonStage(radon_out, self.radon_params, sigma, self.radon_lines, self.radon_lines_params,
                                                       segments_out, rprof_out, self.stack_params, rdef_out, self.defocus_params,
                                                       self.radon_short, short_out, lc, self.radon_wide, wide_out, strip,
                                                       self.radon_null, null_out, fap_out, self.radon_null_scheme, rounds_out)
            if seeing is not None:
                prof_kw["seeing"] = seeing
                if radon is not None:
                    radon.seeing = seeing
            masks = None
            if self.trail_masks:
                masks = prof_kw["masks"] = _MaskStage(masks_out, self.mask_params, self.mask_dir)
            sub = None
            if self.subtract_trails:
                sub = prof_kw["sub"] = _SubStage(sub_out, self.sub_params, self.mask_params, self.clean_dir)
            rounds = None
            if self.rounds:
                rounds = prof_kw["rounds"] = _RoundsStage(trails_out, self.rounds_params)
            preview = None
            if self.previews is not None:
                preview = prof_kw["preview"] = _PreviewStage(previews_out, self.previews, self.preview_params, self.preview_dir)
            streak = None
            if self.streaks:
                sigma = _native.make_sky_params(**self.sky_params).target_sigma if self.normalize else 0.025
                streak = prof_kw["streak"] = _StreakStage(streaks_out, self.streaks_params, sigma)
            if fresh:
                progress.write(header + "\n")
                progress.flush()

            def mark(done_keys):                     # rows first, then the marks: a crash in between repeats a chunk, never loses one
                results.flush()
                errors.flush()
                if profiles is not None:
                    profiles.flush()
                if sky is not None:
                    sky.flush()
                if stars is not None:
                    stars.flush()
                if radon is not None:
                    radon.flush()
                if seeing is not None:                # (after the fits of profiles and radon, which ask it for their frames' seeing)
                    seeing.flush()
                if masks is not None:
                    masks.flush()
                if lc is not None:
                    lc.flush()
                if strip is not None:
                    strip.flush()
                if sub is not None:
                    sub.flush()
                if rounds is not None:
                    rounds.flush()
                if preview is not None:
                    preview.flush()
                if streak is not None:
                    streak.flush()
                progress.write("".join("%s %s %s %s\n" % tuple(k) for k in done_keys))
                progress.flush()

            if batch <= 1:
                for key in keys:
                    process_field(results, errors, *key, self.params_bright, self.params_dim, self.params_removestars, **prof_kw)
                    mark([key])
                if sky is not None:
                    sky.close()
                if radon is not None:
                    radon.close()
                self.last_stats["seconds"] = time.perf_counter() - t_start
                return
            # a chunk = one GPU call: 64 frames keep the link and the GPU busy for plain files; a selection that exists only as
            # .fits.bz2 is decompressed on the GPU a chunk at a time, and that decoder wants thousands of 900 kB blocks at once
            # (~14 per frame): 256 frames per chunk
            if not keys:
                return
            first = sdssfiles.filename("frame", run=keys[0][0], camcol=keys[0][1], field=keys[0][3], filter=keys[0][2])
            compressed = not os.path.exists(first) and os.path.exists(first + ".bz2") and os.environ.get("LFD_BZ2_DEVICE", "1") != "0"
            slots = max(1, min(batch, int(os.environ.get("LFD_LOADER_SLOTS", 256 if compressed else 64)), len(keys)))
            chunks = [keys[i:i + slots] for i in range(0, len(keys), slots)]
            if not chunks:
                return
            shape = _frame_shape(keys)
            # chunks loading at once: one for plain files (the link is the limit), two for selections decompressed on the GPU (two
            # decoders side by side: one chunk's Huffman stage overlaps the other's inverse BWT, loader.FrameLoader)
            depth = max(1, min(int(os.environ.get("LFD_LOADER_DEPTH", 2 if compressed else 1)), len(chunks)))
            with use_context(*shape, inflight=slots) as ctx:
                loader = FrameLoader(ctx, shape, slots, loader_threads, depth=depth, expect_bz2=compressed, catalogs=not self.find_stars)
            self.last_stats.update(chunk_frames=slots, setup_s=time.perf_counter() - t_start)
            try:
                trace = os.environ.get("LFD_LOADER_TRACE") == "1"
                from collections import deque
                with ThreadPoolExecutor(depth, thread_name_prefix="lfd-chunk") as coord:
                    pending, nxt_i = deque(), 0

                    def submit():
                        nonlocal nxt_i
                        j = nxt_i
                        nxt_i += 1
                        pending.append(coord.submit(loader.load, chunks[j], j % (depth + 1), chunks[j + 1] if j + 1 < len(chunks) else None, j))
                    for _ in range(depth):
                        submit()
                    for i, chunk in enumerate(chunks):
                        t0 = time.perf_counter()
                        loaded = pending.popleft().result()
                        t1 = time.perf_counter()
                        # (chunk i sits in buffer i % (depth + 1); the loads in flight fill the other `depth` buffers)
                        if nxt_i < len(chunks):
                            submit()
                        process_loaded(results, errors, loaded, self.params_bright, self.params_dim, self.params_removestars, **prof_kw)
                        mark(chunk)
                        self.last_stats["chunk_done_s"].append(time.perf_counter() - t_start)
                        if trace:
                            print("[loader] chunk %d: waited %.1f ms for its files, GPU call + rows %.1f ms" %
                                  (i, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)), flush=True)
            finally:
                self.last_stats["bz2"] = dict(loader.bz2_stats)
                if sky is not None:
                    sky.close()
                if radon is not None:
                    radon.close()
                loader.close()
                self.last_stats["seconds"] = time.perf_counter() - t_start
