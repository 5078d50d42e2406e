"""Defocus models of a trail's cross-section and their bank on the device (include/lfdmi.h: defocus fit).

The constants keep the names of lfd/analysis/profiles/consts.py.  ``DefocusBank`` builds the bank of model columns with
lfdmi_defocus_bank_create; ``Context.fit_defocus`` / ``BatchDetector.fit_defocus`` fit trail profiles against it.
"""
import ctypes as C
import weakref

import numpy as np

from . import _native

RAD2ARCSEC = 206264.806247
FWHM2SIGMA = 2.436
HEIGHTS = [80., 100., 120., 150.]
RS = [0.1, 0.5, 5, 10]
SEEINGS = [0.67, 1.3455, 1.48, 1.6353]
LSSTSEEING = 0.67
SDSSSEEING = 1.43
LSST = (4180., 2558.)
SDSS = (1250., 585.)

DEFOCUS_DTYPE = _native.DEFOCUS_DTYPE
# what generic_sampler(returnType="grid") reports per model (samplers.py:150-162), plus the bank's validity flag
GRID_DTYPE = np.dtype([("h", "<f8"), ("radius", "<f8"), ("sfwhm", "<f8"), ("dfwhm", "<f8"), ("ofwhm", "<f8"), ("depth", "<f8"),
                       ("valid", "?")])
TRAIL_KEYS = ("pixscale", "prof_half", "prof_step", "wing")
DEFOCUS_COLUMNS = ("run", "camcol", "filter", "field", "status", "h_km", "h_lo", "h_hi", "radius_m", "seeing_arcsec", "shift",
                   "amplitude", "offset", "chi2", "dof", "chi2_focus", "model_ofwhm", "model_depth")


def default_params():
    """lfdmi_default_defocus_params as a dict: heights, radii, seeings (numpy), instrument, ovs, max_shift, delta_chi2 and the
    trail params the bank is built for."""
    p = _native.DefocusParams()
    _native.lib().lfdmi_default_defocus_params(C.byref(p))
    return {"heights": np.array(p.heights[:p.n_h]), "radii": np.array(p.radii[:p.n_r]), "seeings": np.array(p.seeings[:p.n_seeing]),
            "instrument": (p.Ro, p.Ri), "ovs": p.ovs, "max_shift": p.max_shift, "delta_chi2": p.delta_chi2,
            "pixscale": p.pixscale, "prof_half": p.prof_half, "prof_step": p.prof_step, "wing": p.wing}


def make_params(heights=None, radii=None, seeings=None, instrument=SDSS, ovs=None, max_shift=None, delta_chi2=None, **trail_params):
    """(DefocusParams, arrays to keep alive).  trail_params: pixscale, prof_half, prof_step, wing (the trail params of the
    profiles; the others of lfdmi_trail_params are accepted and ignored); delta_chi2 defaults to 1 / prof_step."""
    d = default_params()
    p = _native.DefocusParams()
    _native.lib().lfdmi_default_defocus_params(C.byref(p))
    tp = _native.make_trail_params(**trail_params)   # unknown names raise
    for k in TRAIL_KEYS:
        setattr(p, k, getattr(tp, k))
    ro, ri = instrument
    p.Ro, p.Ri = float(ro), float(ri)
    if ovs is not None:
        p.ovs = int(ovs)
    if max_shift is not None:
        p.max_shift = int(max_shift)
    p.delta_chi2 = 1.0 / p.prof_step if delta_chi2 is None else float(delta_chi2)
    keep = []
    for name, cnt, val in (("heights", "n_h", heights), ("radii", "n_r", radii), ("seeings", "n_seeing", seeings)):
        a = np.ascontiguousarray(d[name] if val is None else np.atleast_1d(np.asarray(val, np.float64)), np.float64)
        if a.ndim != 1 or a.size == 0:
            raise ValueError(f"{name}: a non-empty 1-d grid")
        keep.append(a)
        setattr(p, name, a.ctypes.data_as(C.POINTER(C.c_double)))
        setattr(p, cnt, a.size)
    return p, keep


class DefocusBank:
    """The model columns of every (seeing, height, radius, shift) on ``ctx``'s device (lfdmi_defocus_bank_create).
    ``heights`` km, ``radii`` m, ``seeings`` FWHM arcsec (None: the defaults), ``instrument`` the mirrors' radii in mm;
    ``trail_params`` must be those of the profiles that will be fitted."""

    def __init__(self, ctx, heights=None, radii=None, seeings=None, instrument=SDSS, **trail_params):
        self._b = C.c_void_p()
        self._lib = _native.lib()
        self.ctx = ctx
        p, keep = make_params(heights, radii, seeings, instrument, **trail_params)
        if not getattr(ctx, "_h", None):
            raise ValueError("the context is closed")
        ctx._chk(self._lib.lfdmi_defocus_bank_create(ctx._h, C.byref(p), C.byref(self._b)))
        ctx.__dict__.setdefault("_banks", weakref.WeakSet()).add(self)   # Context.close() closes its banks first
        self.heights, self.radii, self.seeings = (np.array(a) for a in keep)
        self.instrument = (p.Ro, p.Ri)
        self.trail_params = {k: getattr(p, k) for k in TRAIL_KEYS}
        self.ovs, self.max_shift, self.delta_chi2 = p.ovs, p.max_shift, p.delta_chi2
        self.n_h = p.n_h
        nc, nm, nb = C.c_int64(), C.c_int64(), C.c_int32()
        self._lib.lfdmi_defocus_bank_dims(self._b, C.byref(nc), C.byref(nm), C.byref(nb))
        self.n_columns, self.n_models, self.n_bins = nc.value, nm.value, nb.value
        self._grid = None

    def _check(self):
        if not self._b or not getattr(self.ctx, "_h", None):
            raise ValueError("the bank is closed")

    @property
    def grid(self):
        """GRID_DTYPE [n_models], in model order ((i_seeing (n_h + 1) + i_h) n_r + i_r); h = inf for the focus model."""
        if self._grid is None:
            self._check()
            raw = np.zeros(self.n_models, _native.DEFOCUS_MODEL_DTYPE)
            self.ctx._chk(self._lib.lfdmi_defocus_bank_read(self._b, None, _native._ptr(raw)))
            g = np.zeros(self.n_models, GRID_DTYPE)
            for a, b in (("h", "h_km"), ("radius", "radius_m"), ("sfwhm", "sfwhm"), ("dfwhm", "dfwhm"), ("ofwhm", "ofwhm"),
                         ("depth", "depth")):
                g[a] = raw[b]
            g["valid"] = raw["valid"] != 0
            self._grid = g
        return self._grid

    def columns(self):
        """float32 [n_columns, 2K+1]: the centred, unit-norm model columns (0 for invalid models)."""
        self._check()
        out = np.empty((self.n_columns, self.n_bins), np.float32)
        self.ctx._chk(self._lib.lfdmi_defocus_bank_read(self._b, _native._ptr(out), None))
        return out

    def close(self):
        if self._b:
            self._lib.lfdmi_defocus_bank_destroy(self._b)
            self._b = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_row(meta, fit):
    """One defocus.txt row: meta = (run, camcol, filter, field); integers as integers, floats with repr."""
    vals = list(meta) + [int(fit["status"])]
    for k in DEFOCUS_COLUMNS[5:]:
        v = fit[k]
        vals.append(int(v) if k in ("shift", "dof") else repr(float(v)))
    return " ".join(str(v) for v in vals)


def read_defocus(path):
    """defocus.txt -> list of dicts keyed by DEFOCUS_COLUMNS (the header line is skipped)."""
    rows = []
    with open(path) as f:
        for ln in f:
            parts = ln.split()
            if not parts or parts[0] == DEFOCUS_COLUMNS[0]:
                continue
            r = {}
            for k, v in zip(DEFOCUS_COLUMNS, parts):
                if k == "filter":
                    r[k] = v
                elif k in ("run", "camcol", "field", "status", "shift", "dof"):
                    r[k] = int(v)
                else:
                    r[k] = float(v)
            rows.append(r)
    return rows
