"""Frame seeing: the PSF width of a frame from its own stars, for the defocus fit's ``seeing`` (include/lfdmi.h: frame seeing).
``Context.measure_seeing`` is the device call; this module holds the parameters, a one-call helper that runs the source finder
with its records left on the device and then the measurement, the host step, the conversion from the measured width to the
seeing FWHM the defocus bank is built on, and the seeing.txt format of ``DetectTrails(seeing=True)``.
"""
import dataclasses
import math

import numpy as np

from . import _native

STAR_DTYPE = _native.PSF_STAR_DTYPE
FRAME_DTYPE = _native.SEEING_FRAME_DTYPE
OK, NOT_CANDIDATE, CLIPPED, CROWDED, BAD_PIXEL = (_native.PSF_OK, _native.PSF_NOT_CANDIDATE, _native.PSF_CLIPPED, _native.PSF_CROWDED,
                                                  _native.PSF_BAD_PIXEL)
SEEING_OK, SEEING_FEW = _native.SEEING_OK, _native.SEEING_FEW
MAX_SAT = _native.PSF_MAX_SAT
FWHM_PER_SIGMA = 2.3548200450309493            # 2 sqrt(2 ln 2)
BANK_SIGMA_PER_FWHM = 1.035 / 2.436            # the bank's S (include/lfdmi.h: defocus fit, step 1)
SEEING_COLUMNS = ("run", "camcol", "filter", "field", "status", "n_cand", "n_ok", "n_used", "fwhm_px", "fwhm_arcsec",
                  "seeing_arcsec", "scatter", "ell")


@dataclasses.dataclass
class PsfParams:
    """lfdmi_psf_params with its defaults; ``validate`` applies the library's rules without a device."""
    k_peak: float = 50.0
    e_max: float = 0.2
    sat: float = MAX_SAT
    win: int = 7
    gap: int = 2
    ring: int = 3
    iso: int = 12
    rad_max: int = 16
    min_stars: int = 5
    max_used: int = 256

    def as_dict(self):
        return dataclasses.asdict(self)

    def validate(self):
        ranges = {"win": (1, 16), "gap": (0, 8), "ring": (1, 8), "iso": (1, 64), "rad_max": (1, 32), "min_stars": (1, 1024),
                  "max_used": (1, 1024)}
        for name, (lo, hi) in ranges.items():
            v = getattr(self, name)
            if int(v) != v:
                raise ValueError(f"{name} must be an integer")
            if not lo <= v <= hi:
                raise ValueError(f"{name} must be {lo} .. {hi}")
        if not (math.isfinite(self.k_peak) and self.k_peak > 0):
            raise ValueError("k_peak must be positive")
        if not 0.0 <= self.e_max <= 1.0:
            raise ValueError("e_max must be 0 .. 1")
        if not 0.0 < self.sat <= MAX_SAT:
            raise ValueError("sat must be positive and at most %g" % MAX_SAT)
        return self


def default_params():
    """lfdmi_default_psf_params as a PsfParams (read from the library: no GPU needed)."""
    p = _native.make_psf_params()
    return PsfParams(**{k: getattr(p, k) for k, _ in _native.PsfParamsStruct._fields_ if k != "pad"})


def as_params(params):
    """None / dict / PsfParams -> validated dict of lfdmi_psf_params fields"""
    if params is None:
        return {}
    if isinstance(params, PsfParams):
        return params.validate().as_dict()
    unknown = set(params) - {f.name for f in dataclasses.fields(PsfParams)}
    if unknown:
        raise TypeError(f"unknown psf parameter {sorted(unknown)[0]!r}")
    PsfParams(**params).validate()
    return dict(params)


def measure_seeing(ctx, frames, sigma=None, stars_params=None, **params):
    """The source finder with its records left on the device, then ``Context.measure_seeing`` on them: (STAR_DTYPE records
    [n, max_used], FRAME_DTYPE records [n], the finder's frame records [n]).  Host frames are uploaded twice, once by each call;
    pass device frames to avoid that."""
    from . import stars
    q = as_params(params)
    drec, sfrec = ctx.find_stars(frames, sigma=sigma, device_out=True, **stars.as_params(stars_params))
    out, frec = ctx.measure_seeing(frames, drec, sfrec, sigma=sigma, **q)
    return out, frec, sfrec


def star_shape(s):
    """Step 5 for one packed star: None (its sums allow no width) or (width in px, ellipticity)."""
    if s["Q0"] <= 0:
        return None
    q0 = float(s["Q0"])
    mx, my = float(s["Qx"]) / q0, float(s["Qy"]) / q0
    sxx, syy, sxy = float(s["Qxx"]) / q0 - mx * mx, float(s["Qyy"]) / q0 - my * my, float(s["Qxy"]) / q0 - mx * my
    if not sxx > 0.0 or not syy > 0.0:
        return None
    t, d = sxx + syy, sxx - syy
    return FWHM_PER_SIGMA * math.sqrt(t / 2.0), math.sqrt(d * d + 4.0 * (sxy * sxy)) / t


def _lower_median(v):
    v = sorted(v)
    return v[(len(v) - 1) // 2]


def frame_seeing(packed, n_packed, e_max=0.2, min_stars=5):
    """Step 5 on the host: the packed stars [n, max_used] and each frame's n_packed -> a structured array [n] of status,
    n_used, fwhm_px, scatter, ell: the values ``Context.measure_seeing`` puts into its frame records."""
    packed = np.asarray(packed, STAR_DTYPE)
    packed = packed.reshape(1, -1) if packed.ndim == 1 else packed
    n_packed = np.broadcast_to(np.asarray(n_packed, np.int64), (len(packed),))
    out = np.zeros(len(packed), [("status", "<i4"), ("n_used", "<i4"), ("fwhm_px", "<f8"), ("scatter", "<f8"), ("ell", "<f8")])
    for i, row in enumerate(packed):
        shapes = [star_shape(row[k]) for k in range(int(n_packed[i]))]
        used = [s for s in shapes if s is not None and s[1] <= e_max]
        fw = sc = ell = float("nan")
        if used:
            fw = _lower_median([s[0] for s in used])
            sc = 1.4826 * _lower_median([abs(s[0] - fw) for s in used])
            ell = _lower_median([s[1] for s in used])
        out[i] = (SEEING_FEW if len(used) < min_stars else SEEING_OK, len(used), fw, sc, ell)
    return out


def render_bank_psf(seeing, pixscale, half, dy=0.0, dx=0.0):
    """The circular PSF whose line integral is the defocus bank's S for the seeing FWHM ``seeing`` (arcsec): a Gaussian of
    sigma = 1.035 / 2.436 * seeing, integrated over each pixel of a (2 half + 1)^2 stamp, unit flux, centred at (dy, dx) px
    from the stamp's middle pixel.  float64."""
    sg = BANK_SIGMA_PER_FWHM * float(seeing) / float(pixscale) * math.sqrt(2.0)
    edges = np.arange(-half - 0.5, half + 1.0, 1.0)
    cy = np.array([math.erf((e - dy) / sg) for e in edges])
    cx = np.array([math.erf((e - dx) / sg) for e in edges])
    return np.outer(0.5 * np.diff(cy), 0.5 * np.diff(cx))


def stamp_fwhm(stamp, win=7, gap=2, ring=3):
    """The definition's steps 3 and 5 on a noise-free float64 stamp whose middle pixel is the peak: the width in px (the ring's
    mean is taken exactly, not truncated: a rendering has no integer scale)."""
    H = win + gap + ring
    c = stamp.shape[0] // 2
    if stamp.shape[0] != stamp.shape[1] or c < H:
        raise ValueError("stamp_fwhm: a square stamp of half-width >= win + gap + ring")
    sq = stamp[c - H:c + H + 1, c - H:c + H + 1]
    ax = np.arange(-H, H + 1, dtype=np.float64)
    dy, dx = np.meshgrid(ax, ax, indexing="ij")
    d = np.maximum(np.abs(dy), np.abs(dx))
    b = sq[d > win + gap].mean()
    m = d <= win
    p, wx, wy = sq[m] - b, dx[m], dy[m]
    q0 = p.sum()
    mx, my = (p * wx).sum() / q0, (p * wy).sum() / q0
    sxx, syy = (p * wx * wx).sum() / q0 - mx * mx, (p * wy * wy).sum() / q0 - my * my
    return FWHM_PER_SIGMA * math.sqrt((sxx + syy) / 2.0)


def bank_table(pixscale, win, seeings, gap=2, ring=3):
    """What the measurement returns, in px, for the bank's PSF at each seeing of the grid (noise-free, centred on a pixel)."""
    H = win + gap + ring
    return np.array([stamp_fwhm(render_bank_psf(s, pixscale, H), win, gap, ring) for s in np.asarray(seeings, np.float64)])


def to_bank_seeing(fwhm_px, pixscale, win, seeings, gap=2, ring=3):
    """The measured width (px) as the seeing FWHM (arcsec) of the defocus bank: the bank's PSF is rendered at every seeing of
    the grid, this very measurement applied to it, and the monotone table inverted by linear interpolation, clamped at its
    ends.  NaN stays NaN.  Nothing here is fitted: the relation follows from the two definitions."""
    grid = np.sort(np.asarray(seeings, np.float64).reshape(-1))
    tab = bank_table(pixscale, win, grid, gap, ring)
    if len(grid) > 1 and not np.all(np.diff(tab) > 0):
        raise ValueError("to_bank_seeing: the measured width does not grow with the seeing on this grid")
    f = np.asarray(fwhm_px, np.float64)
    out = np.interp(f, tab, grid)
    return np.where(np.isnan(f), np.nan, out) if out.ndim else (float("nan") if math.isnan(float(f)) else float(out))


def format_row(meta, frec, pixscale, seeing_arcsec):
    """One seeing.txt row: meta = (run, camcol, filter, field); frec a FRAME_DTYPE record; seeing_arcsec: ``to_bank_seeing`` of
    its width, NaN for a LFDMI_SEEING_FEW frame."""
    fw = float(frec["fwhm_px"])
    vals = (int(frec["status"]), int(frec["n_cand"]), int(frec["n_ok"]), int(frec["n_used"]), repr(fw), repr(fw * float(pixscale)),
            repr(float(seeing_arcsec)), repr(float(frec["scatter"])), repr(float(frec["ell"])))
    return " ".join(str(v) for v in (*meta, *vals))


def read_seeing(path):
    """seeing.txt -> list of dicts keyed by SEEING_COLUMNS (a header line is skipped)."""
    ints = set(SEEING_COLUMNS[:8]) - {"filter"}
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts or parts[0] == SEEING_COLUMNS[0]:
                continue
            rows.append({k: (v if k == "filter" else int(v) if k in ints else float(v)) for k, v in zip(SEEING_COLUMNS, parts)})
    return rows
