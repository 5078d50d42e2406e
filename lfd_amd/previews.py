"""Frame previews: small 8-bit images of whole frames, binned and stretched on the device (include/lfdmi.h: frame previews).
``Context.frame_previews`` is the device call; this module holds the stretch tables, a one-call helper, the overlay of trail
segments on a preview (host, numpy: the images are small by then), the file names of the reference's image checker, the PNG
writer and the previews.txt format of ``DetectTrails(previews=...)``.
"""
import math
import re

import numpy as np

from . import _native

FRAME_DTYPE = _native.PREVIEW_FRAME_DTYPE
OK, FLAT, EMPTY = _native.PREVIEW_OK, _native.PREVIEW_FLAT, _native.PREVIEW_EMPTY
RANK, GIVEN = _native.PREVIEW_RANK, _native.PREVIEW_GIVEN
LUT = _native.PREVIEW_LUT
BINS = _native.PREVIEW_BINS
EMPTY_CELL = _native.PREVIEW_EMPTY_CELL
LUT_KINDS = ("asinh", "linear", "sqrt")
PREVIEW_COLUMNS = ("run", "camcol", "filter", "field", "status", "bin", "lo", "hi", "n_cells", "n_empty", "file")
# the image checker's name of a frame's picture (restated: frame-{filter}-{run:06d}-{camcol}-{field:04}.{ext})
FILENAME_FORMAT = "frame-{filter}-{run:06d}-{camcol}-{field:04}.{ext}"
_FILENAME_RE = re.compile(r"^frame-([^-]+)-(\d{6,})-(\d+)-(\d{4,})\.(.+)$")


def lut(kind="asinh", softening=0.1):
    """The stretch table of 4096 bytes: level k = 0 .. 4095 stands for x = k / 4095 between the limits.  ``linear``: 255 x;
    ``sqrt``: 255 sqrt(x); ``asinh``: 255 asinh(x / softening) / asinh(1 / softening), nearly linear below ``softening`` and
    logarithmic above it, which keeps a faint trail visible beside a saturated star.  Rounded to the nearest byte."""
    if kind not in LUT_KINDS:
        raise ValueError(f"unknown stretch {kind!r}: one of {LUT_KINDS}")
    x = np.arange(LUT, dtype=np.float64) / (LUT - 1)
    if kind == "sqrt":
        y = np.sqrt(x)
    elif kind == "asinh":
        s = float(softening)
        if not (math.isfinite(s) and s > 0):
            raise ValueError("softening must be positive")
        y = np.arcsinh(x / s) / math.asinh(1.0 / s)
    else:
        y = x
    return np.clip(np.rint(255.0 * y), 0, 255).astype(np.uint8)


def as_params(params):
    """None / dict -> the keywords of ``Context.frame_previews`` that a driver may set (checked without a device)"""
    p = dict(params or {})
    unknown = set(p) - {"bin", "mode", "lo_ppm", "hi_ppm", "limits", "lut", "kind", "softening", "color", "thick"}
    if unknown:
        raise TypeError(f"unknown preview parameter {sorted(unknown)[0]!r}")
    if int(p.get("bin", 4)) not in BINS:
        raise ValueError(f"bin must be one of {BINS}")
    if p.get("mode", "rank") not in ("rank", "given", RANK, GIVEN):
        raise ValueError("mode must be 'rank' or 'given'")
    lo, hi = int(p.get("lo_ppm", 10000)), int(p.get("hi_ppm", 995000))
    if not 0 <= lo <= hi <= 1000000:
        raise ValueError("0 <= lo_ppm <= hi_ppm <= 1000000")
    return p


def frame_previews(ctx, frames, **kw):
    """``Context.frame_previews`` in one call: (uint8 images [n, Hp, Wp], FRAME_DTYPE records [n]); every keyword is the call's."""
    return ctx.frame_previews(frames, **kw)


def overlay(gray, segments, bin, color=(255, 64, 64), thick=1.0):
    """A preview (Hp, Wp) uint8 with the rails of trail segments drawn on it -> RGB (Hp, Wp, 3) uint8.  segments:
    ``masks.SEGMENT_DTYPE`` records (their frame is not looked at).  A cell is marked when its centre, in full-resolution
    flipped coordinates ((i + 0.5) bin - 0.5, (r + 0.5) bin - 0.5), lies on one of a segment's two rails,
    half <= |u| <= half + thick * bin and -cap <= t <= L + cap, with u, t, L and cap as in the trail masks (steps 2 and 3 of
    that section): the trail itself stays visible between the rails.  A bad segment (L == 0, not finite) draws nothing."""
    gray = np.asarray(gray, np.uint8)
    if gray.ndim != 2:
        raise ValueError("overlay: one (Hp, Wp) preview")
    b = int(bin)
    rgb = np.repeat(gray[:, :, None], 3, axis=2)
    hp, wp = gray.shape
    y = ((np.arange(hp, dtype=np.float64) + 0.5) * b - 0.5)[:, None]
    x = ((np.arange(wp, dtype=np.float64) + 0.5) * b - 0.5)[None, :]
    for s in np.asarray(segments, _native.MASK_SEGMENT_DTYPE).reshape(-1):
        x1, y1, x2, y2, half, cap = (float(s[k]) for k in ("x1", "y1", "x2", "y2", "half", "cap"))
        if not all(math.isfinite(v) for v in (x1, y1, x2, y2, half)) or math.isnan(cap) or half < 0 or cap < 0:
            continue
        dx, dy = x2 - x1, y2 - y1
        L = math.sqrt(dx * dx + dy * dy)
        if L == 0:
            continue
        ex, ey = dx / L, dy / L
        nx, ny = -ey, ex
        u = (x - x1) * nx + (y - y1) * ny
        t = (x - x1) * ex + (y - y1) * ey
        au = np.abs(u)
        rail = (au >= half) & (au <= half + float(thick) * b) & (t >= -cap) & (t <= L + cap)
        rgb[rail] = np.asarray(color, np.uint8)
    return rgb


def filename(run, camcol, filter, field, ext="fits.png"):
    """The image checker's file name of a frame's picture: frame-{filter}-{run:06d}-{camcol}-{field:04}.{ext}"""
    return FILENAME_FORMAT.format(filter=filter, run=int(run), camcol=int(camcol), field=int(field), ext=ext)


def parse_filename(name):
    """The inverse of ``filename``: (run, camcol, filter, field, ext) of a file name (its directory is ignored)"""
    m = _FILENAME_RE.match(name.replace("\\", "/").rsplit("/", 1)[-1])
    if not m:
        raise ValueError(f"not a frame picture's name: {name!r}")
    return int(m.group(2)), int(m.group(3)), m.group(1), int(m.group(4)), m.group(5)


def write_png(path, img):
    """A preview (grey) or an overlay (RGB) as an 8-bit PNG"""
    from .detecttrails import debugio
    debugio.write_png(path, img)


def format_row(meta, bin, rec, file):
    """One previews.txt row: meta = (run, camcol, filter, field); rec a FRAME_DTYPE record; lo, hi in the frames' units (repr)"""
    vals = (int(rec["status"]), int(bin), repr(float(rec["lo_f"])), repr(float(rec["hi_f"])), int(rec["n_cells"]), int(rec["n_empty"]), file)
    return " ".join(str(v) for v in (*meta, *vals))


def read_previews(path):
    """previews.txt -> list of dicts keyed by PREVIEW_COLUMNS (a header line is skipped)."""
    ints = {"run", "camcol", "field", "status", "bin", "n_cells", "n_empty"}
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts or parts[0] == PREVIEW_COLUMNS[0]:
                continue
            rows.append({k: (int(v) if k in ints else float(v) if k in ("lo", "hi") else v) for k, v in zip(PREVIEW_COLUMNS, parts)})
    return rows
