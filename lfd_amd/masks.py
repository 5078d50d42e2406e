"""Trail masks: which pixels belong to a trail, as a uint8 plane per frame, and optionally the same pixels filled in the frames
(include/lfdmi.h: trail masks).  ``Context.mask_trails`` is the device call; this module holds the half-width rule, the segments
of every measurement unit's records, a one-call helper, the packed form of a plane and the masks.txt row format.
"""
import numpy as np

from . import _native

SEGMENT_DTYPE = _native.MASK_SEGMENT_DTYPE
STAT_DTYPE = _native.MASK_STAT_DTYPE
OK, BAD_SEGMENT, EMPTY = _native.MASK_OK, _native.MASK_BAD_SEGMENT, _native.MASK_EMPTY
FILLS = tuple(_native.MASK_FILLS)
MASK_COLUMNS = ("run", "camcol", "filter", "field", "source", "line", "x1", "y1", "x2", "y2", "half", "n_pix")


def half_width(fwhm, k_fwhm=2.0, min_half=4.0, grow=2.0, default_half=8.0):
    """The band's half-width in px for a trail of the measured ``fwhm`` (px): max(min_half, k_fwhm * fwhm / 2) + grow, and
    default_half + grow where fwhm is NaN or not positive (no measurement).  k_fwhm = 2 reaches 2.35 sigma of a Gaussian on
    either side before ``grow``."""
    fwhm = float(fwhm)
    if not fwhm > 0.0:                                      # (NaN too)
        return float(default_half) + float(grow)
    return max(float(min_half), float(k_fwhm) * fwhm / 2.0) + float(grow)


def segments(rows, bits=1, cap=0.0, fill=0.0):
    """(frame, x1, y1, x2, y2, half) rows -> SEGMENT_DTYPE records with the given bits, cap and fill"""
    out = np.zeros(len(rows), SEGMENT_DTYPE)
    for i, (f, x1, y1, x2, y2, half) in enumerate(rows):
        out[i]["frame"], out[i]["bits"] = int(f), int(bits)
        out[i]["x1"], out[i]["y1"], out[i]["x2"], out[i]["y2"] = float(x1), float(y1), float(x2), float(y2)
        out[i]["half"], out[i]["cap"], out[i]["fill"] = float(half), float(cap), float(fill)
    return out


def _half_kw(kw):
    unknown = set(kw) - {"k_fwhm", "min_half", "grow", "default_half"}
    if unknown:
        raise TypeError(f"unknown mask parameter {sorted(unknown)[0]!r}")
    return kw


def segments_from_trails(records, frames=None, bits=1, cap=0.0, fill=0.0, **half_kw):
    """Trail records (TRAIL_DTYPE, ``Context.measure_trails``) -> (SEGMENT_DTYPE records, index of each one's record): x1 .. y2
    of every record with status OK, half-width from its fwhm.  frames: the frame of each record (default: its index)."""
    rec = np.asarray(records, _native.TRAIL_DTYPE).reshape(-1)
    frames = np.arange(len(rec)) if frames is None else np.asarray(frames).reshape(-1)
    keep = [i for i, r in enumerate(rec) if int(r["status"]) == _native.TRAIL_OK]
    rows = [(frames[i], rec[i]["x1"], rec[i]["y1"], rec[i]["x2"], rec[i]["y2"], half_width(rec[i]["fwhm"], **_half_kw(half_kw)))
            for i in keep]
    return segments(rows, bits, cap, fill), keep


def segments_from_stack(records, segs, bits=1, cap=0.0, fill=0.0, **half_kw):
    """Stack records (STACK_DTYPE, ``Context.stack_profiles``) and the STACK_SEGMENT_DTYPE segments they were measured on ->
    (SEGMENT_DTYPE records, index of each one's record): the refined x1 .. y2 of every record with status OK on its segment's
    frame, half-width from its fwhm."""
    rec = np.asarray(records, _native.STACK_DTYPE).reshape(-1)
    sg = np.asarray(segs, _native.STACK_SEGMENT_DTYPE).reshape(-1)
    if len(rec) != len(sg):
        raise ValueError(f"{len(rec)} records for {len(sg)} segments")
    keep = [i for i, r in enumerate(rec) if int(r["status"]) == _native.STACK_OK]
    rows = [(sg[i]["frame"], rec[i]["x1"], rec[i]["y1"], rec[i]["x2"], rec[i]["y2"], half_width(rec[i]["fwhm"], **_half_kw(half_kw)))
            for i in keep]
    return segments(rows, bits, cap, fill), keep


def segments_from_radon_lines(lines, n_lines, fwhm=None, bits=1, cap=0.0, fill=0.0, **half_kw):
    """The found lines of ``Radon.search_lines`` (records [n, K], n_lines [n]) -> (SEGMENT_DTYPE records, (frame, line) of each):
    every found line's segment ex1 .. ey2, frames ascending, peel order within a frame.  fwhm: None (the default half-width) or
    one value per found line in that order (NaN: no measurement)."""
    lines = np.asarray(lines)
    if lines.ndim == 1:
        lines = lines[None]
    rows, where = [], []
    for i, nl in enumerate(np.asarray(n_lines).reshape(-1)):
        for k in range(int(nl)):
            r = lines[i, k]
            fw = float("nan") if fwhm is None else fwhm[len(rows)]
            rows.append((i, r["ex1"], r["ey1"], r["ex2"], r["ey2"], half_width(fw, **_half_kw(half_kw))))
            where.append((i, k))
    return segments(rows, bits, cap, fill), where


def segments_from_radon_wide(lines, n_lines, bits=1, cap=0.0, fill=0.0):
    """The found bands of ``Radon.search_wide`` (records [n, K], n_lines [n]) -> (SEGMENT_DTYPE records, (frame, line) of each):
    every found band's segment ex1 .. ey2 on its centre line, frames ascending, peel order within a frame, with
    half = width_px / 2 + 2: the band itself and two pixels beyond either edge."""
    lines = np.asarray(lines)
    if lines.ndim == 1:
        lines = lines[None]
    rows, where = [], []
    for i, nl in enumerate(np.asarray(n_lines).reshape(-1)):
        for k in range(int(nl)):
            r = lines[i, k]
            rows.append((i, r["ex1"], r["ey1"], r["ex2"], r["ey2"], float(r["width_px"]) / 2.0 + 2.0))
            where.append((i, k))
    return segments(rows, bits, cap, fill), where


def segments_from_results(rows, frames=None, fwhm=None, bits=1, cap=0.0, fill=0.0, **half_kw):
    """Results rows (dicts or records with x1 y1 x2 y2: ``results.read_results``, or detection records with found != 0) ->
    SEGMENT_DTYPE records, one per row.  The end points of a results row lie far off the image by construction (the Hough line
    +- 1000 px), which the definition allows: the band covers the line across the frame.  frames: the frame of each row (default:
    its index); fwhm: None or one value per row."""
    out = []
    for i, r in enumerate(rows):
        fw = float("nan") if fwhm is None else fwhm[i]
        out.append((i if frames is None else frames[i], r["x1"], r["y1"], r["x2"], r["y2"], half_width(fw, **_half_kw(half_kw))))
    return segments(out, bits, cap, fill)


def mask_frames(ctx, frames, segs, **kw):
    """``Context.mask_trails`` in one call: (mask, STAT_DTYPE records, counts per frame)."""
    return ctx.mask_trails(frames, segs, **kw)


def pack(mask):
    """uint8 planes (n, h, w) or (h, w) -> (bits, shape): one bit per pixel (set where the byte is not 0), ``np.packbits`` per
    frame, so bits is uint8 [n, ceil(h w / 8)]; shape is the mask's."""
    mask = np.asarray(mask)
    shape = tuple(int(v) for v in mask.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"expected a 2-d plane or a 3-d set of planes, got shape {shape}")
    flat = (mask != 0).reshape(1 if len(shape) == 2 else shape[0], -1)
    return np.packbits(flat, axis=1), shape


def unpack(bits, shape):
    """what ``pack`` returned -> uint8 planes of 0 / 1 of that shape"""
    shape = tuple(int(v) for v in shape)
    npx = shape[-2] * shape[-1]
    bits = np.asarray(bits, np.uint8).reshape(1 if len(shape) == 2 else shape[0], -1)
    return np.unpackbits(bits, axis=1, count=npx).reshape(shape)


def format_row(meta, source, line, seg, n_pix):
    """One masks.txt row: meta = (run, camcol, filter, field), source = ``detect`` or ``radon``, line = the record's place in its
    frame; floats with repr."""
    vals = [repr(float(seg[k])) for k in ("x1", "y1", "x2", "y2", "half")]
    return " ".join(str(v) for v in (*meta, source, int(line), *vals, int(n_pix)))


def read_masks(path):
    """masks.txt (rows only, no header line) -> list of dicts keyed by MASK_COLUMNS."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts:
                continue
            r = {}
            for k, v in zip(MASK_COLUMNS, parts):
                r[k] = v if k in ("filter", "source") else int(v) if k in ("run", "camcol", "field", "line", "n_pix") else float(v)
            rows.append(r)
    return rows
