"""Cross-section tables for ``Context.inject_trails`` (include/lfdmi.h: trail injection), built on the host in double.  A table
is 2M+1 values at offsets (k - M) * step px from the trail's line: the profile as the sky shows it, before the pixel (the pixel
integration is the injection's sub-sampling).  Every builder returns (float64 values, step in px)."""
import math

import numpy as np

from . import _native

INJECT_DTYPE = _native.INJECT_DTYPE
MAX_TABLE = _native.INJECT_MAX_TABLE
RAD2ARCSEC = 206264.806247
FWHM2SIGMA = 2.436


def _check(values, step):
    if len(values) > MAX_TABLE:
        raise ValueError(f"a table of {len(values)} nodes exceeds the {MAX_TABLE} the device holds: use a coarser step")
    return values, step


def gaussian_table(sigma_px, step=0.125, n_sigma=6.0):
    """exp(-u^2 / (2 sigma^2)), peak 1, out to n_sigma sigmas (6: the first node left out is 1.5e-8 of the peak)."""
    if not (sigma_px > 0 and step > 0):
        raise ValueError("sigma_px and step must be positive")
    M = int(math.ceil(n_sigma * sigma_px / step))
    u = np.arange(-M, M + 1, dtype=np.float64) * step
    return _check(np.exp(-(u * u) / (2.0 * sigma_px * sigma_px)), float(step))


def _unit(w):
    return w / w.sum()


def defocus_table(h_km, radius_m=0.0, seeing_fwhm=1.43, Ro=1250.0, Ri=585.0, pixscale=0.396, prof_step=0.1, ovs=8):
    """O (x) D (x) S of include/lfdmi.h ("defocus fit", steps 1-2) on that section's fine grid, without the pixel B and the
    interpolation T: an object of radius ``radius_m`` at ``h_km`` (inf: in focus) seen through mirrors Ro / Ri mm and a seeing
    of ``seeing_fwhm`` arcsec.  Unit sum; the step is prof_step / ovs px (delta = prof_step * pixscale / ovs arcsec)."""
    delta = prof_step * pixscale / ovs
    point = (not np.isfinite(h_km)) or radius_m == 0
    if np.isfinite(h_km):
        to, ti = Ro / (h_km * 1e6) * RAD2ARCSEC, Ri / (h_km * 1e6) * RAD2ARCSEC
        n = int(math.floor(to / delta))
        x = np.arange(-n, n + 1) * delta
        outer = np.sqrt(np.maximum(to * to - x * x, 0.0))
        inner = np.where(np.abs(x) < ti, np.sqrt(np.maximum(ti * ti - x * x, 0.0)), 0.0)
        D = _unit(2.0 / (math.pi * (to * to - ti * ti)) * (outer - inner))
    else:
        D = np.ones(1)
    if point:
        O = np.ones(1)
    else:
        rho = radius_m / (2 * h_km * 1000) * RAD2ARCSEC
        n = int(math.floor(rho / delta))
        x = np.arange(-n, n + 1) * delta
        O = _unit(2.0 * np.sqrt(np.maximum(rho * rho - x * x, 0.0)) / (math.pi * rho * rho))
    sigma = 1.035 / FWHM2SIGMA * seeing_fwhm
    n = int(math.floor(4 * sigma / delta))
    x = np.arange(-n, n + 1) * delta
    S = _unit(np.exp(-(x * x) / (2 * sigma * sigma)))
    return _check(np.convolve(np.convolve(O, D), S), prof_step / ovs)


def normalise_peak(table):
    """The table scaled to peak 1, so that a trail's ``amplitude`` is its peak in frame units (before the pixel)."""
    t = np.asarray(table, np.float64)
    peak = t.max()
    if not peak > 0:
        raise ValueError("the table has no positive value")
    return t / peak


def integral(table, step):
    """The table's trapezoid integral in table units x px: the flux a unit length of a trail of amplitude 1 adds."""
    t = np.asarray(table, np.float64)
    return float(step * (t.sum() - 0.5 * (t[0] + t[-1])))


def make_trails(n):
    """n zeroed INJECT_DTYPE records with unbounded extents"""
    tr = np.zeros(n, INJECT_DTYPE)
    tr["t0"], tr["t1"] = -np.inf, np.inf
    return tr
