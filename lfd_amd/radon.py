"""Faint-trail search: the line of largest signal-to-noise of a whole frame by the dyadic fast Radon transform -- for trails
that are faint in every pixel but long, which the detector cannot see (include/lfdmi.h: faint-trail search).  ``_native.Radon``
is the device handle; this module holds the parameters, the host conversion of a working line to the frame (usable without a
device), a one-call helper and the radon.txt format of ``DetectTrails(radon=True)``; for several lines per frame (steps 7 - 9 of
the definition): ``RadonLinesParams``, the dyadic path, a segment's end points, ``search_lines`` and the radon_segments.txt format;
for short trails, scored on every dyadic level (steps 10 - 12): ``RadonShortParams``, ``search_short`` and the radon_short.txt
format; for wide trails, scored as sliding bands of neighbouring lines (steps 13 - 16): ``RadonWideParams``, ``search_wide``
and the radon_wide.txt format; for a frame's own noise ceiling (null peaks, steps 17 - 20): ``null_peaks``, ``false_alarm``,
``null_threshold`` and the radon_null.txt and radon_fap.txt formats; for nulls that leave the pixels in place and the nulls of
the peel rounds (steps 21 - 22): the ``scheme`` and ``peel`` arguments of ``null_peaks``, ``shift_scheme_for``, ``peel_from_lines``,
``null_rounds`` and the radon_null_rounds.txt format.
"""
import dataclasses
import math

import numpy as np

from . import _native

RADON_DTYPE = _native.RADON_DTYPE
RADON_LINE_DTYPE = _native.RADON_LINE_DTYPE
RADON_SHORT_DTYPE = _native.RADON_SHORT_DTYPE
RADON_WIDE_DTYPE = _native.RADON_WIDE_DTYPE
OK, NO_LINE = _native.RADON_OK, _native.RADON_NO_LINE
DEFAULT_SIGMA = 0.025
RADON_COLUMNS = ("run", "camcol", "filter", "field", "x1", "y1", "x2", "y2", "snr", "n_pix")
SEGMENT_COLUMNS = ("run", "camcol", "filter", "field", "line", "ex1", "ey1", "ex2", "ey2", "seg_snr", "seg_n_pix")
SHORT_COLUMNS = ("run", "camcol", "filter", "field", "line", "level", "strip", "snr", "n_pix", "ex1", "ey1", "ex2", "ey2", "seg_snr",
                 "seg_n_pix")
WIDE_COLUMNS = ("run", "camcol", "filter", "field", "line", "width", "width_px", "snr", "n_pix", "ex1", "ey1", "ex2", "ey2", "seg_snr",
                "seg_n_pix")
NULL_KINDS = ("lines", "short", "wide")
NULL_SCHEMES = tuple(_native.RADON_NULL_SCHEMES)
RADON_PEEL_DTYPE = _native.RADON_PEEL_DTYPE
NULL_ROUNDS_COLUMNS = ("run", "camcol", "filter", "field", "kind", "round", "K", "null_min", "null_median", "null_max")
NULL_COLUMNS = ("run", "camcol", "filter", "field", "kind", "K", "null_min", "null_median", "null_max")
FAP_COLUMNS = ("run", "camcol", "filter", "field", "kind", "line", "snr", "n_ge", "K", "fap")
INT_COLUMNS = frozenset(("run", "camcol", "field", "line", "level", "strip", "width", "n_pix", "seg_n_pix"))   # of every file here


class _Params:
    """What the parameter classes share; those of the peeling searches also the rules of their common fields."""

    def as_dict(self):
        return dataclasses.asdict(self)

    def _integers(self):
        for f in dataclasses.fields(self):
            if f.type is int and int(getattr(self, f.name)) != getattr(self, f.name):
                raise ValueError(f"{f.name} must be an integer")

    def _peel_rules(self, seg_max, seg_text, threshold=None):
        """max_lines, peel_halfwidth, min_seg (1 .. seg_max if that is known, worded ``seg_text``) and the field ``threshold``"""
        if not 1 <= self.max_lines <= _native.RADON_MAX_LINES:
            raise ValueError("max_lines must be 1 .. %d" % _native.RADON_MAX_LINES)
        if self.peel_halfwidth < 0:
            raise ValueError("peel_halfwidth must be >= 0")
        if self.min_seg < 1 or (seg_max is not None and self.min_seg > seg_max):
            raise ValueError(f"min_seg must be 1 .. {seg_text}")
        if threshold and not (math.isfinite(getattr(self, threshold)) and getattr(self, threshold) > 0):
            raise ValueError(f"{threshold} must be finite and positive")
        return self


@dataclasses.dataclass
class RadonParams(_Params):
    """lfdmi_radon_params with its defaults; ``validate`` applies the library's rules without a device."""
    bin: int = 2
    clip: float = 0.125
    min_len: int = 256
    threshold: float = 8.0

    def validate(self):
        if self.bin not in (1, 2, 4):
            raise ValueError("bin must be 1, 2 or 4")
        if not (math.isfinite(self.clip) and self.clip > 0):
            raise ValueError("clip must be positive")
        if int(self.min_len) != self.min_len or self.min_len < 1:
            raise ValueError("min_len must be an integer >= 1")
        if math.isnan(self.threshold):
            raise ValueError("threshold must be a number")
        return self


@dataclasses.dataclass
class RadonLinesParams(_Params):
    """lfdmi_radon_lines_params with its defaults; ``validate`` applies the library's rules without a device (``min_len``: the
    handle's, which bounds ``min_seg``)."""
    max_lines: int = 4
    peel_halfwidth: int = 8
    min_seg: int = 64

    def validate(self, min_len=None):
        self._integers()
        return self._peel_rules(min_len, "min_len")


@dataclasses.dataclass
class RadonShortParams(_Params):
    """lfdmi_radon_short_params with its defaults; ``validate`` applies the library's rules without a device (``bin``: the
    handle's, which bounds ``min_seg`` by min_strip * bin * bin / 2)."""
    min_strip: int = 64
    max_lines: int = 4
    peel_halfwidth: int = 8
    min_seg: int = 32
    short_threshold: float = 8.5

    def validate(self, bin=None):
        self._integers()
        if self.min_strip < 64 or self.min_strip & (self.min_strip - 1):
            raise ValueError("min_strip must be a power of two >= 64")
        return self._peel_rules(None if bin is None else self.min_strip * bin * bin // 2, "min_strip * bin * bin / 2", "short_threshold")


@dataclasses.dataclass
class RadonWideParams(_Params):
    """lfdmi_radon_wide_params with its defaults; ``validate`` applies the library's rules without a device (``min_len``: the
    handle's, which bounds ``min_seg``)."""
    max_width: int = 8
    max_lines: int = 4
    peel_halfwidth: int = 8
    min_seg: int = 64
    wide_threshold: float = 8.0

    def validate(self, min_len=None):
        self._integers()
        if not 1 <= self.max_width <= _native.RADON_MAX_WIDTH or self.max_width & (self.max_width - 1):
            raise ValueError("max_width must be a power of two, 1 .. %d" % _native.RADON_MAX_WIDTH)
        return self._peel_rules(min_len, "min_len", "wide_threshold")


def _defaults(cls, made):
    return cls(**{f.name: getattr(made, f.name) for f in dataclasses.fields(cls)})


def default_params():
    """lfdmi_default_radon_params as a RadonParams (read from the library: no GPU needed)."""
    return _defaults(RadonParams, _native.make_radon_params())


def default_lines_params():
    """lfdmi_default_radon_lines_params as a RadonLinesParams (read from the library: no GPU needed)."""
    return _defaults(RadonLinesParams, _native.make_radon_lines_params())


def default_short_params():
    """lfdmi_default_radon_short_params as a RadonShortParams (read from the library: no GPU needed)."""
    return _defaults(RadonShortParams, _native.make_radon_short_params())


def default_wide_params():
    """lfdmi_default_radon_wide_params as a RadonWideParams (read from the library: no GPU needed)."""
    return _defaults(RadonWideParams, _native.make_radon_wide_params())


def _as_params(cls, word, params, *bound):
    """None / dict / ``cls`` -> validated dict of its fields (``bound``: what ``cls.validate`` takes)"""
    if params is None:
        return {}
    if isinstance(params, cls):
        return params.validate(*bound).as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(cls)}
    if unknown:
        raise TypeError(f"unknown {word} parameter {sorted(unknown)[0]!r}")
    cls(**params).validate(*bound)
    return dict(params)


def as_params(params):
    """None / dict / RadonParams -> validated dict of lfdmi_radon_params fields"""
    return _as_params(RadonParams, "radon", params)


def as_lines_params(params, min_len=None):
    """None / dict / RadonLinesParams -> validated dict of lfdmi_radon_lines_params fields"""
    return _as_params(RadonLinesParams, "radon lines", params, min_len)


def as_short_params(params, bin=None):
    """None / dict / RadonShortParams -> validated dict of lfdmi_radon_short_params fields"""
    return _as_params(RadonShortParams, "radon short", params, bin)


def as_wide_params(params, min_len=None):
    """None / dict / RadonWideParams -> validated dict of lfdmi_radon_wide_params fields"""
    return _as_params(RadonWideParams, "radon wide", params, min_len)


def working_dims(shape, bin):
    """(Hb, Wb, P of orientations 0 and 1, P of orientations 2 and 3)"""
    h, w = int(shape[0]), int(shape[1])
    hb, wb = -(-h // bin), -(-w // bin)
    return hb, wb, 1 << max(0, (wb - 1).bit_length()), 1 << max(0, (hb - 1).bit_length())


def _mapping(q, shape, bin):
    """Step 6's mapping for orientation q (q and bin checked): (P, C, the function (c, r) -> (x, y)) -- a working point in the
    detection records' coordinates (x = column, y = row of the flipped frame)"""
    if q not in (0, 1, 2, 3):
        raise ValueError("q must be 0 .. 3")
    if bin not in (1, 2, 4):
        raise ValueError("bin must be 1, 2 or 4")
    hb, wb, p01, p23 = working_dims(shape, bin)

    def point(c, r):
        i, j = ((c, r), (c, hb - 1 - r), (r, c), (wb - 1 - r, c))[q]
        return bin * i + (bin - 1) / 2.0, bin * j + (bin - 1) / 2.0
    return (p01, wb, point) if q < 2 else (p23, hb, point)


def line_of(q, y0, s, shape, bin):
    """Step 6 of the definition: the working line (q, y0, s) of frames of ``shape`` searched at ``bin`` as (x1, y1, x2, y2, rho,
    theta) in the detection records' coordinates (x = column, y = row of the flipped frame); theta in [0, pi) and
    x cos(theta) + y sin(theta) = rho."""
    P, _, point = _mapping(q, shape, bin)
    (x1, y1), (x2, y2) = point(0, int(y0)), point(P - 1, int(y0) + int(s))
    theta = math.atan2(-(x2 - x1), y2 - y1)
    if theta < 0.0:
        theta += math.pi
    if theta >= math.pi:
        theta -= math.pi
    return x1, y1, x2, y2, x1 * math.cos(theta) + y1 * math.sin(theta), theta


def dyadic_path(s, P):
    """Step 7 of the definition: d(c; s, P) for c = 0 .. P-1, the row offset of the dyadic line of slope s in each column of a
    working array of width P (a power of two): line (q, y0, s) is the cells Q[y0 + d[c]][c]."""
    s, P = int(s), int(P)
    if P < 1 or P & (P - 1) or not 0 <= s < P:
        raise ValueError("P must be a power of two and 0 <= s < P")
    c = np.arange(P, dtype=np.int64)
    d = np.zeros(P, np.int64)
    n = P >> 1
    while n:
        d += np.where(c & n, (s + 1) >> 1, 0)
        n >>= 1
        s >>= 1
    return d


def segment_points(q, y0, s, c1, c2, shape, bin):
    """Step 9's end points: the working points (c1, y0 + d(c1)) and (c2, y0 + d(c2)) of line (q, y0, s) as (ex1, ey1, ex2, ey2)
    in the detection records' coordinates."""
    P, C, point = _mapping(q, shape, bin)
    if not 0 <= c1 <= c2 < C:
        raise ValueError("0 <= c1 <= c2 < C")
    d = dyadic_path(s, P)
    return tuple(v for c in (int(c1), int(c2)) for v in point(c, int(y0) + int(d[c])))


def _search(ctx, frames, rp, call):
    """``call(handle, frames)`` on a handle made for (n, h, w) or (h, w) ``frames`` with the RadonParams fields ``rp``, created
    and destroyed here"""
    arr = frames if _native._is_dev(frames) or isinstance(frames, _native.DeviceFrames) else np.asarray(frames)
    shp = tuple(arr.shape)
    n, h, w = (1, *shp) if len(shp) == 2 else shp
    with _native.Radon(ctx, (h, w), max_frames=max(1, min(n, ctx.max_inflight)), **rp) as r:
        return call(r, arr)


def _split(params, cls):
    """the keyword arguments that are not fields of ``cls``, and those that are"""
    names = {f.name for f in dataclasses.fields(cls)}
    return {k: v for k, v in params.items() if k not in names}, {k: v for k, v in params.items() if k in names}


def search_lines(ctx, frames, sigma=None, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx`` for several lines each: (RADON_LINE_DTYPE records [n, max_lines], n_lines
    [n]).  ``params``: fields of RadonParams and of RadonLinesParams.  The handle is created and destroyed per call."""
    rp, lp = _split(params, RadonLinesParams)
    lp, rp = as_lines_params(lp), as_params(rp)
    return _search(ctx, frames, rp, lambda r, arr: r.search_lines(arr, sigma=sigma, **lp))


def search_short(ctx, frames, sigma=None, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx`` for short trails: (RADON_SHORT_DTYPE records [n, max_lines], n_lines [n]).
    ``params``: fields of RadonParams and of RadonShortParams.  The handle is created and destroyed per call."""
    rp, sp = _split(params, RadonShortParams)
    rp = as_params(rp)
    sp = as_short_params(sp, rp.get("bin", RadonParams.bin))
    return _search(ctx, frames, rp, lambda r, arr: r.search_short(arr, sigma=sigma, **sp))


def search_wide(ctx, frames, sigma=None, plain=False, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx`` for wide trails: (RADON_WIDE_DTYPE records [n, max_lines], n_lines [n]), and
    with ``plain`` the RADON_DTYPE records of the plain search as a third item.  ``params``: fields of RadonParams and of
    RadonWideParams.  The handle is created and destroyed per call."""
    rp, wp = _split(params, RadonWideParams)
    rp = as_params(rp)
    wp = as_wide_params(wp, rp.get("min_len", RadonParams.min_len))
    return _search(ctx, frames, rp, lambda r, arr: r.search_wide(arr, sigma=sigma, plain=plain, **wp))


def search_frames(ctx, frames, sigma=None, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx``: RADON_DTYPE records, one per frame.  For repeated calls keep a
    ``_native.Radon`` handle instead: this one is created and destroyed per call."""
    return _search(ctx, frames, as_params(params), lambda r, arr: r.search(arr, sigma=sigma))


def _null_params(K, kind, scheme, peel, params):
    """the checks ``null_peaks`` makes before the device: (RadonParams fields, the kind's parameters)"""
    if kind not in NULL_KINDS:
        raise ValueError("kind: 'lines', 'short' or 'wide'")
    if scheme not in NULL_SCHEMES:
        raise ValueError("scheme: 'scramble', 'signflip', 'rowshift' or 'colshift'")
    if not 1 <= int(K) <= _native.RADON_NULL_MAX:
        raise ValueError("K must be 1 .. %d" % _native.RADON_NULL_MAX)
    if peel is not None and scheme != "signflip":
        raise ValueError("peel records need scheme='signflip': the other schemes move the pixels from under the band")
    kp = {}
    if kind == "short":
        params, kp = _split(params, RadonShortParams)
    elif kind == "wide":
        params, kp = _split(params, RadonWideParams)
    elif scheme != "scramble" or peel is not None:       # (the scramble without peel records takes no lines parameters)
        params, kp = _split(params, RadonLinesParams)
    rp = as_params(params)
    if kind == "short":
        kp = as_short_params(kp, rp.get("bin", RadonParams.bin))
    elif kind == "wide":
        kp = as_wide_params(kp, rp.get("min_len", RadonParams.min_len))
    elif kp:
        kp = as_lines_params(kp, rp.get("min_len", RadonParams.min_len))
    return rp, kp


def null_peaks(ctx, frames, K=16, kind="lines", sigma=None, seeds=None, scheme="scramble", peel=None, **params):
    """The null peaks of (n, h, w) or (h, w) frames on ``ctx`` (include/lfdmi.h: faint-trail search, null peaks): float32
    [n, K], the best score of the ``kind`` search ("lines", "short", "wide") of K null realisations of every frame -- the
    frame's own noise ceiling.  ``params``: fields of RadonParams and of the kind's parameters.  seeds: None (frame f has seed
    f) or one uint64 per frame.  scheme: "scramble" (every pixel drawn from the whole frame), "signflip" (every pixel in its
    place, its sign by a coin), "rowshift" / "colshift" (every row / column rotated by its own offset; ``shift_scheme_for``).
    peel (signflip only): RADON_PEEL_DTYPE records [n, n_peel] (``peel_from_lines``), blotted before the search with the
    kind's ``peel_halfwidth`` (kind "lines": a field of RadonLinesParams).  A realisation without a candidate has the peak 0.
    The handle is created and destroyed per call; ``_native.Radon.null`` returns the whole records."""
    rp, kp = _null_params(K, kind, scheme, peel, params)
    return _search(ctx, frames, rp, lambda r, arr: np.ascontiguousarray(
        r.null(arr, K=K, kind=kind, sigma=sigma, seeds=seeds, scheme=scheme, peel=peel, **kp)["snr"]))


def shift_scheme_for(q):
    """The shift scheme that destroys a line of orientation q: "colshift" for q = 0, 1, whose lines cross the columns (the row
    shift would leave a trail along the rows whole), "rowshift" for q = 2, 3."""
    if q not in (0, 1, 2, 3):
        raise ValueError("q must be 0 .. 3")
    return "colshift" if q < 2 else "rowshift"


def peel_from_lines(lines, n_lines, upto):
    """RADON_PEEL_DTYPE [n, upto]: the first min(n_lines, upto) found lines of every frame from the records [n, max_lines] of
    ``search_lines``, ``search_short`` or ``search_wide`` (width: the band's, 1 where the record has none); the places after
    them have width 0, no line."""
    lines = np.asarray(lines)
    n_lines = np.asarray(n_lines).reshape(-1)
    upto = int(upto)
    if lines.ndim != 2 or len(n_lines) != lines.shape[0] or not 0 <= upto <= min(lines.shape[1], _native.RADON_MAX_LINES):
        raise ValueError("lines: records [n, max_lines], n_lines: [n], upto: 0 .. max_lines")
    out = np.zeros((lines.shape[0], upto), RADON_PEEL_DTYPE)
    has = np.arange(upto)[None, :] < n_lines[:, None]
    for k in ("q", "y0", "s"):
        out[k] = np.where(has, lines[k][:, :upto], 0)
    out["width"] = np.where(has, lines["width"][:, :upto] if "width" in lines.dtype.names else 1, 0)
    return out


def null_rounds(ctx, frames, lines, n_lines, K=16, kind="lines", sigma=None, seeds=None, **params):
    """The null peaks of every peel round of (n, h, w) frames on ``ctx``: float32 [n, max_lines, K] from the records
    ``lines`` [n, max_lines] and ``n_lines`` of the kind's search of these frames.  Round k is the "signflip" null with the
    frame's lines 0 .. k-1 blotted as the search blotted them (``params`` must be that search's: ``peel_halfwidth`` among
    them), which is the null the search's round k -- line k -- has to be held against.  NaN where the frame never ran round
    k: the search ran it iff k <= n_lines.  One handle and one call per round; the frames of a round keep their seeds."""
    lines = np.asarray(lines)
    n_lines = np.asarray(n_lines).reshape(-1)
    rp, kp = _null_params(K, kind, "signflip", lines, params)
    n, max_lines = lines.shape

    def run(r, arr):
        if arr.ndim == 2:
            arr = arr[None]
        sg = None if sigma is None else np.broadcast_to(np.asarray(sigma, np.float32), (n,))
        sd = np.arange(n, dtype=np.uint64) if seeds is None else np.asarray(seeds, np.uint64).reshape(-1)
        out = np.full((n, max_lines, int(K)), np.nan, np.float32)
        for k in range(max_lines):
            ran = np.flatnonzero(n_lines >= k)
            if not len(ran):
                break
            part = arr if len(ran) == n else arr[torch_index(arr, ran)]
            pl = peel_from_lines(lines[ran], n_lines[ran], k) if k else None
            out[ran, k] = r.null(part, K=K, kind=kind, sigma=None if sg is None else np.ascontiguousarray(sg[ran]), seeds=sd[ran],
                                 scheme="signflip", peel=pl, **kp)["snr"]
        return out
    return _search(ctx, frames, rp, run)


def torch_index(arr, idx):
    """``idx`` as an index of the frames ``arr``: a device tensor takes a tensor on its device"""
    if _native._is_dev(arr):
        import torch
        return torch.as_tensor(idx, device=arr.device)
    return idx


def false_alarm(snr, null_snr):
    """(1 + #{null >= snr}) / (K + 1): the standard estimate of the chance that a frame without a trail reaches ``snr``, from
    that frame's K null peaks; never 0 (K nulls cannot show less than 1 / (K + 1))."""
    null = np.asarray(null_snr, np.float32).reshape(-1)
    if null.size < 1:
        raise ValueError("null_snr: at least one null peak")
    return (1 + int(np.count_nonzero(null >= np.float32(snr)))) / (null.size + 1)


def null_threshold(null_snr, margin=1.5):
    """``margin`` times the largest null peak: the rule the default thresholds follow on their noise crops (include/lfdmi.h,
    steps 5 and 12), applied to a frame's (or a set of frames') own null peaks."""
    null = np.asarray(null_snr, np.float32).reshape(-1)
    if null.size < 1:
        raise ValueError("null_snr: at least one null peak")
    return float(margin) * float(null.max())


def null_seed(run, camcol, filter, field):
    """The seed of a frame's null peaks in ``DetectTrails(radon_null=K)``: a fixed 64-bit mix of (run, camcol, filter index,
    field), so a resumed run and any rank split give the same rows.  filter: one of 'ugriz' or its index."""
    fi = "ugriz".index(filter) if isinstance(filter, str) else int(filter)
    x = 0
    for v in (int(run), int(camcol), fi, int(field)):
        x = _splitmix64((x ^ (v & _MASK64)) & _MASK64)
    return x


_MASK64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def format_null_row(meta, kind, null_snr):
    """One radon_null.txt row: meta = (run, camcol, filter, field), the kind and its K null peaks' minimum, median and maximum
    (float32 values, floats with repr; the median of an even K is the float32 mean of the middle two)"""
    null = np.sort(np.asarray(null_snr, np.float32).reshape(-1))
    return " ".join(str(v) for v in (*meta, kind, null.size, repr(float(null[0])), repr(float(np.median(null))), repr(float(null[-1]))))


def format_fap_row(meta, kind, line, snr, null_snr):
    """One radon_fap.txt row of a found line: meta, the kind, the line's place in peel order, its snr, how many of the frame's K
    null peaks reach it, K and ``false_alarm``"""
    null = np.asarray(null_snr, np.float32).reshape(-1)
    n_ge = int(np.count_nonzero(null >= np.float32(snr)))
    return " ".join(str(v) for v in (*meta, kind, int(line), repr(float(snr)), n_ge, null.size, repr(false_alarm(snr, null))))


def format_null_rounds_row(meta, kind, round, null_snr):
    """One radon_null_rounds.txt row: ``format_null_row`` with the peel round after the kind"""
    null = np.sort(np.asarray(null_snr, np.float32).reshape(-1))
    return " ".join(str(v) for v in (*meta, kind, int(round), null.size, repr(float(null[0])), repr(float(np.median(null))),
                                     repr(float(null[-1]))))


def read_null_rounds(path):
    """radon_null_rounds.txt (rows only, no header line) -> list of dicts keyed by NULL_ROUNDS_COLUMNS"""
    return _read_kinds(path, NULL_ROUNDS_COLUMNS)


def read_null(path):
    """radon_null.txt (rows only, no header line) -> list of dicts keyed by NULL_COLUMNS"""
    return _read_kinds(path, NULL_COLUMNS)


def read_fap(path):
    """radon_fap.txt (rows only, no header line) -> list of dicts keyed by FAP_COLUMNS"""
    return _read_kinds(path, FAP_COLUMNS)


def _read_kinds(path, columns):
    ints = INT_COLUMNS | {"K", "n_ge", "round"}
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if parts:
                rows.append({k: v if k in ("filter", "kind") else int(v) if k in ints else float(v) for k, v in zip(columns, parts)})
    return rows


def _format(columns, meta, line, rec):
    """one row of the file with ``columns``: meta, then ``line`` and the record's fields, floats with repr"""
    return " ".join(str(v) for v in (*meta, *(int(line) if k == "line" else int(rec[k]) if k in INT_COLUMNS else repr(float(rec[k]))
                                              for k in columns[4:])))


def _read(path, columns):
    """a file of rows of ``columns`` (rows only, no header line) -> list of dicts keyed by them"""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if parts:
                rows.append({k: v if k == "filter" else int(v) if k in INT_COLUMNS else float(v) for k, v in zip(columns, parts)})
    return rows


def format_row(meta, rec):
    """One radon.txt row: meta = (run, camcol, filter, field); floats with repr."""
    return _format(RADON_COLUMNS, meta, None, rec)


def read_radon(path):
    """radon.txt (rows only, no header line) -> list of dicts keyed by RADON_COLUMNS."""
    return _read(path, RADON_COLUMNS)


def format_segment_row(meta, line, rec):
    """One radon_segments.txt row: meta = (run, camcol, filter, field), line = the record's place in peel order; floats with
    repr."""
    return _format(SEGMENT_COLUMNS, meta, line, rec)


def read_segments(path):
    """radon_segments.txt (rows only, no header line) -> list of dicts keyed by SEGMENT_COLUMNS."""
    return _read(path, SEGMENT_COLUMNS)


def format_short_row(meta, line, rec):
    """One radon_short.txt row: meta = (run, camcol, filter, field), line = the record's place in peel order; floats with repr."""
    return _format(SHORT_COLUMNS, meta, line, rec)


def read_short(path):
    """radon_short.txt (rows only, no header line) -> list of dicts keyed by SHORT_COLUMNS."""
    return _read(path, SHORT_COLUMNS)


def format_wide_row(meta, line, rec):
    """One radon_wide.txt row: meta = (run, camcol, filter, field), line = the record's place in peel order; floats with repr."""
    return _format(WIDE_COLUMNS, meta, line, rec)


def read_wide(path):
    """radon_wide.txt (rows only, no header line) -> list of dicts keyed by WIDE_COLUMNS."""
    return _read(path, WIDE_COLUMNS)
