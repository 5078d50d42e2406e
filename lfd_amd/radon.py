"""Faint-trail search: the line of largest signal-to-noise of a whole frame by the dyadic fast Radon transform -- for trails
that are faint in every pixel but long, which the detector cannot see (include/lfdmi.h: faint-trail search).  ``_native.Radon``
is the device handle; this module holds the parameters, the host conversion of a working line to the frame (usable without a
device), a one-call helper and the radon.txt format of ``DetectTrails(radon=True)``; for several lines per frame (steps 7 - 9 of
the definition): ``RadonLinesParams``, the dyadic path, a segment's end points, ``search_lines`` and the radon_segments.txt format;
for short trails, scored on every dyadic level (steps 10 - 12): ``RadonShortParams``, ``search_short`` and the radon_short.txt
format; for wide trails, scored as sliding bands of neighbouring lines (steps 13 - 16): ``RadonWideParams``, ``search_wide``
and the radon_wide.txt format.
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


@dataclasses.dataclass
class RadonParams:
    """lfdmi_radon_params with its defaults; ``validate`` applies the library's rules without a device."""
    bin: int = 2
    clip: float = 0.125
    min_len: int = 256
    threshold: float = 8.0

    def as_dict(self):
        return dataclasses.asdict(self)

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


def default_params():
    """lfdmi_default_radon_params as a RadonParams (read from the library: no GPU needed)."""
    p = _native.make_radon_params()
    return RadonParams(**{k: getattr(p, k) for k, _ in _native.RadonParamsStruct._fields_})


def as_params(params):
    """None / dict / RadonParams -> validated dict of lfdmi_radon_params fields"""
    if params is None:
        return {}
    if isinstance(params, RadonParams):
        return params.validate().as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(RadonParams)}
    if unknown:
        raise TypeError(f"unknown radon parameter {sorted(unknown)[0]!r}")
    RadonParams(**params).validate()
    return dict(params)


@dataclasses.dataclass
class RadonLinesParams:
    """lfdmi_radon_lines_params with its defaults; ``validate`` applies the library's rules without a device (``min_len``: the
    handle's, which bounds ``min_seg``)."""
    max_lines: int = 4
    peel_halfwidth: int = 8
    min_seg: int = 64

    def as_dict(self):
        return dataclasses.asdict(self)

    def validate(self, min_len=None):
        for name in ("max_lines", "peel_halfwidth", "min_seg"):
            if int(getattr(self, name)) != getattr(self, name):
                raise ValueError(f"{name} must be an integer")
        if not 1 <= self.max_lines <= _native.RADON_MAX_LINES:
            raise ValueError("max_lines must be 1 .. %d" % _native.RADON_MAX_LINES)
        if self.peel_halfwidth < 0:
            raise ValueError("peel_halfwidth must be >= 0")
        if self.min_seg < 1 or (min_len is not None and self.min_seg > min_len):
            raise ValueError("min_seg must be 1 .. min_len")
        return self


def default_lines_params():
    """lfdmi_default_radon_lines_params as a RadonLinesParams (read from the library: no GPU needed)."""
    p = _native.make_radon_lines_params()
    return RadonLinesParams(**{k: getattr(p, k) for k, _ in _native.RadonLinesParamsStruct._fields_})


def as_lines_params(params, min_len=None):
    """None / dict / RadonLinesParams -> validated dict of lfdmi_radon_lines_params fields"""
    if params is None:
        return {}
    if isinstance(params, RadonLinesParams):
        return params.validate(min_len).as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(RadonLinesParams)}
    if unknown:
        raise TypeError(f"unknown radon lines parameter {sorted(unknown)[0]!r}")
    RadonLinesParams(**params).validate(min_len)
    return dict(params)


@dataclasses.dataclass
class RadonShortParams:
    """lfdmi_radon_short_params with its defaults; ``validate`` applies the library's rules without a device (``bin``: the
    handle's, which bounds ``min_seg`` by min_strip * bin * bin / 2)."""
    min_strip: int = 64
    max_lines: int = 4
    peel_halfwidth: int = 8
    min_seg: int = 32
    short_threshold: float = 8.5

    def as_dict(self):
        return dataclasses.asdict(self)

    def validate(self, bin=None):
        for name in ("min_strip", "max_lines", "peel_halfwidth", "min_seg"):
            if int(getattr(self, name)) != getattr(self, name):
                raise ValueError(f"{name} must be an integer")
        if self.min_strip < 64 or self.min_strip & (self.min_strip - 1):
            raise ValueError("min_strip must be a power of two >= 64")
        if not 1 <= self.max_lines <= _native.RADON_MAX_LINES:
            raise ValueError("max_lines must be 1 .. %d" % _native.RADON_MAX_LINES)
        if self.peel_halfwidth < 0:
            raise ValueError("peel_halfwidth must be >= 0")
        if self.min_seg < 1 or (bin is not None and self.min_seg > self.min_strip * bin * bin // 2):
            raise ValueError("min_seg must be 1 .. min_strip * bin * bin / 2")
        if not (math.isfinite(self.short_threshold) and self.short_threshold > 0):
            raise ValueError("short_threshold must be finite and positive")
        return self


def default_short_params():
    """lfdmi_default_radon_short_params as a RadonShortParams (read from the library: no GPU needed)."""
    p = _native.make_radon_short_params()
    return RadonShortParams(**{k: getattr(p, k) for k, _ in _native.RadonShortParamsStruct._fields_ if k != "pad"})


def as_short_params(params, bin=None):
    """None / dict / RadonShortParams -> validated dict of lfdmi_radon_short_params fields"""
    if params is None:
        return {}
    if isinstance(params, RadonShortParams):
        return params.validate(bin).as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(RadonShortParams)}
    if unknown:
        raise TypeError(f"unknown radon short parameter {sorted(unknown)[0]!r}")
    RadonShortParams(**params).validate(bin)
    return dict(params)


@dataclasses.dataclass
class RadonWideParams:
    """lfdmi_radon_wide_params with its defaults; ``validate`` applies the library's rules without a device (``min_len``: the
    handle's, which bounds ``min_seg``)."""
    max_width: int = 8
    max_lines: int = 4
    peel_halfwidth: int = 8
    min_seg: int = 64
    wide_threshold: float = 8.0

    def as_dict(self):
        return dataclasses.asdict(self)

    def validate(self, min_len=None):
        for name in ("max_width", "max_lines", "peel_halfwidth", "min_seg"):
            if int(getattr(self, name)) != getattr(self, name):
                raise ValueError(f"{name} must be an integer")
        if not 1 <= self.max_width <= _native.RADON_MAX_WIDTH or self.max_width & (self.max_width - 1):
            raise ValueError("max_width must be a power of two, 1 .. %d" % _native.RADON_MAX_WIDTH)
        if not 1 <= self.max_lines <= _native.RADON_MAX_LINES:
            raise ValueError("max_lines must be 1 .. %d" % _native.RADON_MAX_LINES)
        if self.peel_halfwidth < 0:
            raise ValueError("peel_halfwidth must be >= 0")
        if self.min_seg < 1 or (min_len is not None and self.min_seg > min_len):
            raise ValueError("min_seg must be 1 .. min_len")
        if not (math.isfinite(self.wide_threshold) and self.wide_threshold > 0):
            raise ValueError("wide_threshold must be finite and positive")
        return self


def default_wide_params():
    """lfdmi_default_radon_wide_params as a RadonWideParams (read from the library: no GPU needed)."""
    p = _native.make_radon_wide_params()
    return RadonWideParams(**{k: getattr(p, k) for k, _ in _native.RadonWideParamsStruct._fields_ if k != "pad"})


def as_wide_params(params, min_len=None):
    """None / dict / RadonWideParams -> validated dict of lfdmi_radon_wide_params fields"""
    if params is None:
        return {}
    if isinstance(params, RadonWideParams):
        return params.validate(min_len).as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(RadonWideParams)}
    if unknown:
        raise TypeError(f"unknown radon wide parameter {sorted(unknown)[0]!r}")
    RadonWideParams(**params).validate(min_len)
    return dict(params)


def working_dims(shape, bin):
    """(Hb, Wb, P of orientations 0 and 1, P of orientations 2 and 3)"""
    h, w = int(shape[0]), int(shape[1])
    hb, wb = -(-h // bin), -(-w // bin)
    return hb, wb, 1 << max(0, (wb - 1).bit_length()), 1 << max(0, (hb - 1).bit_length())


def line_of(q, y0, s, shape, bin):
    """Step 6 of the definition: the working line (q, y0, s) of frames of ``shape`` searched at ``bin`` as (x1, y1, x2, y2, rho,
    theta) in the detection records' coordinates (x = column, y = row of the flipped frame); theta in [0, pi) and
    x cos(theta) + y sin(theta) = rho."""
    if q not in (0, 1, 2, 3):
        raise ValueError("q must be 0 .. 3")
    if bin not in (1, 2, 4):
        raise ValueError("bin must be 1, 2 or 4")
    hb, wb, p01, p23 = working_dims(shape, bin)
    P = p01 if q < 2 else p23
    pts = []
    for c, r in ((0, int(y0)), (P - 1, int(y0) + int(s))):
        i, j = ((c, r), (c, hb - 1 - r), (r, c), (wb - 1 - r, c))[q]
        pts.append((bin * i + (bin - 1) / 2.0, bin * j + (bin - 1) / 2.0))
    (x1, y1), (x2, y2) = pts
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
    if q not in (0, 1, 2, 3):
        raise ValueError("q must be 0 .. 3")
    if bin not in (1, 2, 4):
        raise ValueError("bin must be 1, 2 or 4")
    hb, wb, p01, p23 = working_dims(shape, bin)
    P, C = (p01, wb) if q < 2 else (p23, hb)
    if not 0 <= c1 <= c2 < C:
        raise ValueError("0 <= c1 <= c2 < C")
    d = dyadic_path(s, P)
    out = []
    for c in (int(c1), int(c2)):
        r = int(y0) + int(d[c])
        i, j = ((c, r), (c, hb - 1 - r), (r, c), (wb - 1 - r, c))[q]
        out += [bin * i + (bin - 1) / 2.0, bin * j + (bin - 1) / 2.0]
    return tuple(out)


def search_lines(ctx, frames, sigma=None, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx`` for several lines each: (RADON_LINE_DTYPE records [n, max_lines], n_lines
    [n]).  ``params``: fields of RadonParams and of RadonLinesParams.  The handle is created and destroyed per call."""
    lnames = {f.name for f in dataclasses.fields(RadonLinesParams)}
    lp = as_lines_params({k: v for k, v in params.items() if k in lnames})
    rp = as_params({k: v for k, v in params.items() if k not in lnames})
    arr = frames if _native._is_dev(frames) or isinstance(frames, _native.DeviceFrames) else np.asarray(frames)
    shp = tuple(arr.shape)
    n, h, w = (1, *shp) if len(shp) == 2 else shp
    with _native.Radon(ctx, (h, w), max_frames=max(1, min(n, ctx.max_inflight)), **rp) as r:
        return r.search_lines(arr, sigma=sigma, **lp)


def search_short(ctx, frames, sigma=None, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx`` for short trails: (RADON_SHORT_DTYPE records [n, max_lines], n_lines [n]).
    ``params``: fields of RadonParams and of RadonShortParams.  The handle is created and destroyed per call."""
    snames = {f.name for f in dataclasses.fields(RadonShortParams)}
    rp = as_params({k: v for k, v in params.items() if k not in snames})
    sp = as_short_params({k: v for k, v in params.items() if k in snames}, rp.get("bin", RadonParams.bin))
    arr = frames if _native._is_dev(frames) or isinstance(frames, _native.DeviceFrames) else np.asarray(frames)
    shp = tuple(arr.shape)
    n, h, w = (1, *shp) if len(shp) == 2 else shp
    with _native.Radon(ctx, (h, w), max_frames=max(1, min(n, ctx.max_inflight)), **rp) as r:
        return r.search_short(arr, sigma=sigma, **sp)


def search_wide(ctx, frames, sigma=None, plain=False, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx`` for wide trails: (RADON_WIDE_DTYPE records [n, max_lines], n_lines [n]), and
    with ``plain`` the RADON_DTYPE records of the plain search as a third item.  ``params``: fields of RadonParams and of
    RadonWideParams.  The handle is created and destroyed per call."""
    wnames = {f.name for f in dataclasses.fields(RadonWideParams)}
    rp = as_params({k: v for k, v in params.items() if k not in wnames})
    wp = as_wide_params({k: v for k, v in params.items() if k in wnames}, rp.get("min_len", RadonParams.min_len))
    arr = frames if _native._is_dev(frames) or isinstance(frames, _native.DeviceFrames) else np.asarray(frames)
    shp = tuple(arr.shape)
    n, h, w = (1, *shp) if len(shp) == 2 else shp
    with _native.Radon(ctx, (h, w), max_frames=max(1, min(n, ctx.max_inflight)), **rp) as r:
        return r.search_wide(arr, sigma=sigma, plain=plain, **wp)


def search_frames(ctx, frames, sigma=None, **params):
    """Search (n, h, w) or (h, w) frames on ``ctx``: RADON_DTYPE records, one per frame.  For repeated calls keep a
    ``_native.Radon`` handle instead: this one is created and destroyed per call."""
    arr = frames if _native._is_dev(frames) or isinstance(frames, _native.DeviceFrames) else np.asarray(frames)
    shp = tuple(arr.shape)
    n, h, w = (1, *shp) if len(shp) == 2 else shp
    with _native.Radon(ctx, (h, w), max_frames=max(1, min(n, ctx.max_inflight)), **as_params(params)) as r:
        return r.search(arr, sigma=sigma)


def format_row(meta, rec):
    """One radon.txt row: meta = (run, camcol, filter, field); floats with repr."""
    return " ".join(str(v) for v in (*meta, repr(float(rec["x1"])), repr(float(rec["y1"])), repr(float(rec["x2"])),
                                      repr(float(rec["y2"])), repr(float(rec["snr"])), int(rec["n_pix"])))


def read_radon(path):
    """radon.txt (rows only, no header line) -> list of dicts keyed by RADON_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            r = {}
            for k, v in zip(RADON_COLUMNS, parts):
                r[k] = v if k == "filter" else int(v) if k in ("run", "camcol", "field", "n_pix") else float(v)
            rows.append(r)
    return rows


def format_segment_row(meta, line, rec):
    """One radon_segments.txt row: meta = (run, camcol, filter, field), line = the record's place in peel order; floats with
    repr."""
    return " ".join(str(v) for v in (*meta, int(line), repr(float(rec["ex1"])), repr(float(rec["ey1"])), repr(float(rec["ex2"])),
                                      repr(float(rec["ey2"])), repr(float(rec["seg_snr"])), int(rec["seg_n_pix"])))


def read_segments(path):
    """radon_segments.txt (rows only, no header line) -> list of dicts keyed by SEGMENT_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            r = {}
            for k, v in zip(SEGMENT_COLUMNS, parts):
                r[k] = v if k == "filter" else int(v) if k in ("run", "camcol", "field", "line", "seg_n_pix") else float(v)
            rows.append(r)
    return rows


def format_short_row(meta, line, rec):
    """One radon_short.txt row: meta = (run, camcol, filter, field), line = the record's place in peel order; floats with repr."""
    return " ".join(str(v) for v in (*meta, int(line), int(rec["level"]), int(rec["strip"]), repr(float(rec["snr"])), int(rec["n_pix"]),
                                      repr(float(rec["ex1"])), repr(float(rec["ey1"])), repr(float(rec["ex2"])),
                                      repr(float(rec["ey2"])), repr(float(rec["seg_snr"])), int(rec["seg_n_pix"])))


def read_short(path):
    """radon_short.txt (rows only, no header line) -> list of dicts keyed by SHORT_COLUMNS."""
    ints = ("run", "camcol", "field", "line", "level", "strip", "n_pix", "seg_n_pix")
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            r = {}
            for k, v in zip(SHORT_COLUMNS, parts):
                r[k] = v if k == "filter" else int(v) if k in ints else float(v)
            rows.append(r)
    return rows


def format_wide_row(meta, line, rec):
    """One radon_wide.txt row: meta = (run, camcol, filter, field), line = the record's place in peel order; floats with repr."""
    return " ".join(str(v) for v in (*meta, int(line), int(rec["width"]), repr(float(rec["width_px"])), repr(float(rec["snr"])),
                                      int(rec["n_pix"]), repr(float(rec["ex1"])), repr(float(rec["ey1"])), repr(float(rec["ex2"])),
                                      repr(float(rec["ey2"])), repr(float(rec["seg_snr"])), int(rec["seg_n_pix"])))


def read_wide(path):
    """radon_wide.txt (rows only, no header line) -> list of dicts keyed by WIDE_COLUMNS."""
    ints = ("run", "camcol", "field", "line", "width", "n_pix", "seg_n_pix")
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            r = {}
            for k, v in zip(WIDE_COLUMNS, parts):
                r[k] = v if k == "filter" else int(v) if k in ints else float(v)
            rows.append(r)
    return rows
