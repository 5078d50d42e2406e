"""The frames, lines and parameters of tests/test_gpu_trail_edges.py, shared with the CPU test of their conditions in
tests/test_trail_cases_model.py.  Every case is one small frame (64 .. 333 px on a side, built from a seed), the float32
rho / theta of its detection record, trail parameters off their defaults, an optional catalogue, the status the restatement
(tests/trail_ref.py) has to reach on it, a note of what it is there for, and, where that can be read off the result, a
predicate `prop(record, profile)` that says so.  Coordinates are the records': x = column, y = row of the flipped frame."""
import functools
import math

import numpy as np

import trail_ref as T

PI2 = float(np.float32(math.pi / 2))
GROUPS = ("corners", "geometry", "ties", "bad", "final", "mask")
# remove_stars parameters of the catalogue cases: a square's half-side is PETROTH90 + 10 px, or 4 px for PETROTH90 = 0
RS = dict(filter="r", defaultxy=4, maxxy=60, pixscale=1.0, magcount=3, maxmagdiff=3,
          filter_caps={"u": 22.0, "g": 22.2, "r": 22.2, "i": 21.3, "z": 20.5})
CASES = {}


def case(name, group, frame, rho, theta, status=T.OK, note="", prop=None, cat=None, found=1, **params):
    assert name not in CASES and group in GROUPS
    CASES[name] = dict(name=name, group=group, make=frame, rho=np.float32(rho), theta=np.float32(theta), status=status, note=note,
                       prop=prop, cat=cat, found=found, params=params)


@functools.lru_cache(maxsize=None)
def frame(name):
    """the case's frame (buffer orientation): built once, shared, never changed"""
    f = np.ascontiguousarray(CASES[name]["make"](), np.float32)
    f.setflags(write=False)
    return f


def by_group(group):
    return [c for c in CASES.values() if c["group"] == group]


def call_key(c):
    """cases with the same key go into one call: frame shape and parameter set"""
    return frame(c["name"]).shape + tuple(sorted(c["params"].items()))


def calls(group=None):
    """lists of cases (of one group), one list per call of the GPU test"""
    out = {}
    for c in CASES.values():
        if group is None or c["group"] == group:
            out.setdefault(call_key(c), []).append(c)
    return list(out.values())


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def dist(h, w, rho, theta):
    """signed distance of every pixel (buffer orientation) from the line x cos(theta) + y sin(theta) = rho"""
    y = (h - 1 - np.arange(h, dtype=np.float64))[:, None]
    x = np.arange(w, dtype=np.float64)[None, :]
    return x * math.cos(theta) + y * math.sin(theta) - rho


def gauss(h, w, rho, theta, sigma=1.5, amp=1.0):
    d = dist(h, w, rho, theta)
    return (amp * np.exp(-d * d / (2 * sigma * sigma))).astype(np.float32)


def noise(h, w, seed, sigma=0.02):
    return np.random.default_rng(seed).normal(0.0, sigma, (h, w)).astype(np.float32)


def trail(h, w, seed, rho, theta, sigma=1.5, amp=1.0, sky=0.02):
    return lambda: noise(h, w, seed, sky) + gauss(h, w, rho, theta, sigma, amp)


def rows(f, y0, y1):
    """the buffer rows of flipped rows y0 .. y1-1"""
    h = f.shape[0]
    return f[h - y1:h - y0]


def centre_line(h, w, theta):
    """rho of the line of normal angle theta through the frame's centre"""
    return (w - 1) / 2 * math.cos(theta) + (h - 1) / 2 * math.sin(theta)


SMALL = dict(half_width=6, wing=2, prof_half=4.0, prof_step=0.5)   # K = 8

# ---- parameter corners ------------------------------------------------------------------------------------------------------------
case("all_min", "corners", trail(64, 65, 1, 30.3, 0.05, sigma=0.6), 30.3, 0.05,
     note="every parameter at its lower bound: 3 offsets, 2 positions per segment, 3 bins, no refit",
     prop=lambda r, p: len(p) == 3 and r["n_seg"] >= 30,
     half_width=1, seg_len=2, wing=1, prof_half=1.0, prof_step=1.0, n_iter=0)
case("all_max", "corners", trail(200, 333, 2, 101.2, PI2 + 0.013, sigma=2.5), 100.0, PI2 + 0.01,
     note="every parameter at its upper bound: 129 offsets of which 128 are wings, 1025 bins that are all wing bins, 16 refits",
     prop=lambda r, p: len(p) == 1025 and r["n_seg"] == 5,
     half_width=64, seg_len=64, wing=64, prof_half=64.0, prof_step=0.125, n_iter=16)

LEN_THETA, LEN_W = 0.04, 64


def length_line(h, theta, L):
    """(rho, npos, nseg) of the line of normal angle theta through the centre of an h x 64 frame"""
    rho = float(np.float32(centre_line(h, LEN_W, theta)))
    th = float(np.float32(theta))
    _, npos, nseg = T.positions(h, LEN_W, [rho * math.cos(th), rho * math.sin(th)], [-math.sin(th), math.cos(th)], L)
    return rho, npos, nseg


def length_cases(L):
    """One frame height per L >= 31, so the cases of one L share a call: the smallest height >= 64 at which the line at
    LEN_THETA has two full segments and the first remainder; the other remainders come from steeper lines, which are longer.
    A partial segment of one or two positions (L = 2, 3) would lose its outer offsets to the border on a steep line, so there
    every remainder has a height of its own."""
    rems = [r for r in (L // 2 - 1, L // 2, L // 2 + 1) if r < L]

    def height(rem):
        return next(h for h in range(64, 334) if length_line(h, LEN_THETA, L)[1] >= 2 * L and length_line(h, LEN_THETA, L)[1] % L == rem)

    for rem in rems:
        h, theta = height(rem if L < 31 else rems[0]), LEN_THETA
        full = length_line(h, LEN_THETA, L)[1] // L
        if L >= 31 and rem != rems[0]:
            fits = [t for t in np.arange(LEN_THETA, 0.35, 0.001) if length_line(h, t, L)[1] == full * L + rem]
            theta = fits[len(fits) // 2]                                    # well inside: the refit must not change the length
        rho, npos, nseg = length_line(h, theta, L)
        kept = 2 * rem >= L and rem > 0
        name = f"len_L{L}_rem{rem}"
        case(name, "corners", trail(h, LEN_W, 100 * L + rem, rho, theta), rho, theta,
             note=f"L = {L}: lanes >= L pad the sort; a last partial segment of {rem} positions is {'kept' if kept else 'dropped'}",
             prop=lambda r, p, nseg=nseg, n=npos if kept else full * L: (r["n_seg"], r["n_pos"]) == (nseg, n),
             seg_len=L, n_iter=1, **SMALL)
        CASES[name].update(rem=rem, kept=kept, L=L)


for _L in (2, 3, 31, 32, 33, 63, 64):
    length_cases(_L)

WING_TH = 2.0
for _wing in (1, 7, 8):
    case(f"wing_{_wing}", "corners", trail(96, 100, 30 + _wing, centre_line(96, 100, WING_TH) + 0.8, WING_TH + 0.004),
         centre_line(96, 100, WING_TH), WING_TH,
         note=f"wing = {_wing} of R = 8: {2 * _wing} of 17 offsets are wings (trail_wing_idx), and so are the bins |u| >= {8 - _wing}",
         prop=lambda r, p: r["n_seg"] == 3 and r["noise"] > 0.0,      # the model test: both depend on the wing width
         half_width=8, wing=_wing, seg_len=32, prof_half=8.0, prof_step=0.25, n_iter=2)
case("k_sig_0", "corners", trail(96, 100, 40, centre_line(96, 100, 1.0) + 0.5, 1.0, amp=0.008), centre_line(96, 100, 1.0), 1.0,
     note="k_sig = 0: segments with 0 < A < 5 sd are significant (the model test: TOO_FAINT at the default k_sig)",
     prop=lambda r, p: r["n_seg"] >= 2, seg_len=16, n_iter=2, k_sig=0.0, **SMALL)
case("k_sig_huge", "corners", trail(96, 100, 41, centre_line(96, 100, 1.0) + 0.5, 1.0), centre_line(96, 100, 1.0), 1.0,
     status=T.TOO_FAINT, note="a k_sig no segment passes", seg_len=16, n_iter=2, k_sig=1e9, **SMALL)
case("not_found_a", "corners", trail(96, 100, 42, 50.0, 1.0), 50.0, 1.0, status=T.NOT_FOUND, found=0,
     note="a record without a detection among measured ones", seg_len=16, n_iter=2, k_sig=0.0, **SMALL)

# ---- geometry -----------------------------------------------------------------------------------------------------------------------
GEO = dict(seg_len=16, n_iter=2, **SMALL)
case("theta_0", "geometry", trail(96, 65, 50, 30.4, 0.0), 30.0, 0.0, note="theta = 0 exactly: d.x is -0.0, no position bound from x",
     prop=lambda r, p: r["n_seg"] == 6 and abs(r["x1"] - r["x2"]) < 0.5 and abs(r["x1"] - 30.4) < 0.2, **GEO)
case("theta_pi2", "geometry", trail(64, 100, 51, 30.4, PI2), 30.0, PI2, note="theta = float32(pi/2): d.y is -4.4e-8, not 0",
     prop=lambda r, p: r["n_seg"] == 6 and abs(r["y1"] - r["y2"]) < 0.5 and abs(r["y1"] - 30.4) < 0.2, **GEO)
case("wide_333", "geometry", trail(64, 333, 52, 31.0, PI2 - 0.02), 30.5, PI2 - 0.021, note="w = 333, 64 rows: 21 segments, the last of 12 positions",
     prop=lambda r, p: (r["n_seg"], r["n_pos"]) == (21, 332), **GEO)


def edge_frame(h, w, seed):
    def make():
        f = noise(h, w, seed)
        f[:, 0] += 1
        f[:, w - 1] += 1
        f[h - 1, :] += 1
        return f
    return make


case("column_0", "geometry", edge_frame(96, 100, 53), 0.0, 0.0, status=T.TOO_FAINT,
     note="a line along column 0: every sample at u < 0 is outside the frame, every segment has NaN offsets", **GEO)
case("column_last", "geometry", edge_frame(96, 100, 53), 99.0, 0.0, status=T.TOO_FAINT,
     note="a line along column w-1: every sample at u >= 0 needs column w", **GEO)
case("row_0", "geometry", edge_frame(96, 100, 53), 0.0, PI2, status=T.TOO_FAINT,
     note="a line along row 0 of the flipped frame (the buffer's last row)", **GEO)
DIAG_TH = math.atan2(332.0, -95.0)
case("diagonal", "geometry", trail(96, 333, 54, 0.3, DIAG_TH), 0.0, DIAG_TH,
     note="through the corners (0, 0) and (w-1, h-1): the end segments lose offsets to both borders",
     prop=lambda r, p: r["n_seg"] < 21, **GEO)
ANTI_TH, ANTI_RHO = math.atan2(99.0, 99.0), 99.0 * 99.0 / math.hypot(99.0, 99.0)
case("anti_diagonal", "geometry", trail(100, 100, 55, ANTI_RHO + 0.3, ANTI_TH), ANTI_RHO, ANTI_TH,
     note="through the corners (0, h-1) and (w-1, 0) of a square frame", prop=lambda r, p: r["min_valid"] < r["n_pos"] - 4, **GEO)
case("npos_2L_minus_1", "geometry", trail(65, 64, 56, 30.0, 0.0), 30.0, 0.0, status=T.TOO_SHORT,
     note="npos = 65 = 2L - 1", seg_len=33, n_iter=1, **SMALL)
case("npos_2L", "geometry", trail(66, 64, 57, 30.0, 0.0), 30.0, 0.0, note="npos = 66 = 2L",
     prop=lambda r, p: (r["n_seg"], r["n_pos"]) == (2, 66), seg_len=33, n_iter=1, **SMALL)
# a line that cuts a corner with 66 positions; the trail lies 2 px nearer the corner, where the refitted line has 62 < 2L
ROT_TH, ROT_RHO = math.pi / 4, 99.0 * math.sqrt(2.0) - 32.9
case("refit_too_short", "geometry", trail(100, 100, 58, ROT_RHO + 2.0, ROT_TH, sigma=1.2), ROT_RHO, ROT_TH, status=T.TOO_SHORT,
     note="npos >= 2L on the start line, < 2L after the first refit (trail_range in k_trail_fit)",
     half_width=4, wing=1, prof_half=4.0, prof_step=0.5, seg_len=32, n_iter=3)

# ---- ties and signs -----------------------------------------------------------------------------------------------------------------
TIES = dict(seg_len=16, n_iter=2, k_sig=2.0, **SMALL)


def quantised(h, w, seed, rho, theta):
    def make():
        f = np.rint(np.random.default_rng(seed).normal(0.0, 1.0, (h, w))).astype(np.float32)   # -3 .. 3, with -0.0
        return np.where(np.abs(dist(h, w, rho, theta)) < 1.5, f + np.float32(6.0), f)                 # keeps the -0.0
    return make


case("quantised_vertical", "ties", quantised(96, 100, 60, 40.0, 0.0), 40.0, 0.0,
     note="integer levels, some negative, sampled a refit's fraction of a pixel beside the pixels: few distinct samples",
     prop=lambda r, p: r["background"] == 0.0 and abs(r["peak"] - 6.0) < 0.01, **TIES)
case("quantised_on_pixels", "ties", quantised(96, 100, 60, 40.0, 0.0), 40.0, 0.0,
     note="the same without a refit: every sample is a pixel, every median is taken among ties and is an integer",
     prop=lambda r, p: np.array_equal(p, np.rint(p)) and r["peak"] == 6.0, **dict(TIES, n_iter=0))
case("quantised_tilted", "ties", quantised(96, 100, 61, centre_line(96, 100, 0.3), 0.3), centre_line(96, 100, 0.3) + 0.4, 0.3,
     note="integer levels under bilinear weights", prop=lambda r, p: r["n_seg"] == 6 and 5.5 < r["peak"] < 6.5, **TIES)


def signed_zeros():
    h, w = 96, 100
    rng = np.random.default_rng(62)
    f = -(1.0 + rng.integers(0, 2, (h, w))).astype(np.float32)
    on = np.abs(dist(h, w, 40.0, 0.0)) < 1.5
    z = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    return np.where(on, z, f).astype(np.float32)


case("signed_zeros", "ties", signed_zeros, 40.0, 0.0,
     note="-0.0 and +0.0 pixels under the trail, negative sky: the radix keys of both zeros and of negative values",
     prop=lambda r, p: r["peak"] == -r["background"] > 0 and (p == r["peak"]).sum() >= 3, **TIES)      # the peak bins' median is a zero
case("constant", "ties", lambda: np.full((96, 100), 0.7, np.float32), 40.0, 0.0, status=T.TOO_FAINT,
     note="a constant frame: sd = 0 and A = 0 in every segment, A > k_sig * sd on equality", **TIES)
case("constant_k_sig_0", "ties", lambda: np.full((96, 100), 0.7, np.float32), 40.0, 0.3, status=T.TOO_FAINT,
     note="the same with k_sig = 0 on a tilted line: A > 0 decides", seg_len=16, n_iter=2, k_sig=0.0, **SMALL)


def runs_frame(spans):
    """a noiseless sky with a trail along column 40.3 over the given flipped rows only"""
    def make():
        f = np.full((96, 100), 0.25, np.float32)
        g = gauss(96, 100, 40.3, 0.0, sigma=1.0)
        for y0, y1 in spans:
            rows(f, y0, y1)[:] += rows(g, y0, y1)
        return f
    return make


case("two_equal_runs", "ties", runs_frame([(0, 32), (48, 80)]), 40.0, 0.0,
     note="segments 0-1 and 3-4 significant, 2 and 5 not: two runs of equal length, the first wins",
     prop=lambda r, p: r["n_seg"] == 2 and r["y1"] < 16.0 and r["y2"] < 40.0, seg_len=16, n_iter=2, **SMALL)
case("one_segment", "ties", runs_frame([(16, 32)]), 40.0, 0.0, status=T.TOO_FAINT,
     note="a single significant segment is no extent", seg_len=16, n_iter=2, **SMALL)

def k_sig_on_equality(A, sd):
    """k_sig = A / sd, where its double product with sd is exactly A and that of the next lower double is less"""
    k = A / sd
    assert k * sd == A and float(np.nextafter(k, 0.0)) * sd < A
    return k


def columns():
    """constant columns around column 40: m_s(u) = 4 at u = 0, wings (-1, 0 | 1, 1) with median 0 and MAD 1, 0 elsewhere"""
    f = np.zeros((96, 100), np.float32)
    f[:, 40], f[:, 34], f[:, 45], f[:, 46] = 4.0, -1.0, 1.0, 1.0
    return f


K_EQ = k_sig_on_equality(4.0, 1.4826 * 1.0)
EQ = dict(half_width=6, wing=2, prof_half=4.0, prof_step=1.0, seg_len=32, n_iter=1)
case("sigma_on_equality", "ties", columns, 40.0, 0.0, status=T.TOO_FAINT,
     note="A = 4 and k_sig * sd = 4 exactly in every segment: A > k_sig * sd is false", k_sig=K_EQ, **EQ)
case("sigma_just_below", "ties", columns, 40.0, 0.0, note="k_sig one ulp lower: every segment is significant",
     prop=lambda r, p: r["n_seg"] == 3 and r["peak"] == 4.0, k_sig=float(np.nextafter(K_EQ, 0.0)), **EQ)

# ---- bad samples ---------------------------------------------------------------------------------------------------------------------
BAD = dict(half_width=3, wing=2, prof_half=8.0, prof_step=0.5, seg_len=32, n_iter=2)


def dead_column(col):
    def make():
        f = trail(96, 100, 70 + col, 40.2, 0.0)().copy()
        f[0::2, col] = np.nan
        f[1::2, col] = np.inf
        f[2::6, col] = -np.inf
        return f
    return make


case("dead_bin", "bad", dead_column(45), 40.0, 0.0,
     note="a NaN / inf column outside the refinement window: the bins 4 <= u < 6 have no valid sample, the others do",
     prop=lambda r, p: r["min_valid"] == 0 and np.isnan(p[16 + 8:16 + 12]).all() and np.isnan(p).sum() == 4, **BAD)
case("dead_wing_bin", "bad", dead_column(47), 40.0, 0.0,
     note="the same in the wing bins 6 <= u < 8: background and noise skip NaN bins",
     prop=lambda r, p: r["min_valid"] == 0 and np.isnan(p[16 + 12:16 + 16]).all() and np.isnan(p).sum() == 4, **BAD)


def overflow():
    th = 0.2
    f = trail(96, 100, 72, centre_line(96, 100, th), th)().copy()
    c, s, rho = math.cos(th), math.sin(th), centre_line(96, 100, th)
    for t, big in ((-30, 3.0e38), (-5, -3.0e38), (22, 3.3e38)):
        x, y = int(49.5 - t * s), int(47.5 + t * c)
        f[95 - y, x], f[95 - y, x + 1], f[95 - y - 1, x] = big, -big, -big
    return f


case("overflow", "bad", overflow, centre_line(96, 100, 0.2) + 0.3, 0.2,
     note="finite taps near +-FLT_MAX: their bilinear differences overflow, the samples are +-inf (valid) or NaN (not)",
     prop=lambda r, p: np.isfinite(p).all() and r["min_valid"] < r["n_pos"] - 1,
     half_width=6, wing=2, prof_half=4.0, prof_step=0.5, seg_len=32, n_iter=2)


def one_valid():
    f = trail(64, 100, 73, 40.2, 0.0)().copy()
    for y in (24, 25, 26, 29, 30, 31):
        rows(f, y, y + 1)[:] = np.nan
    return f


case("one_valid_sample", "bad", one_valid, 40.0, 0.0,
     note="segment 3 of 8 positions keeps one valid sample per offset (t = 27): a median of one",
     prop=lambda r, p: r["n_seg"] == 8 and r["min_valid"] <= 64 - 9, seg_len=8, n_iter=2, **SMALL)


# ---- k_trail_final's paths ---------------------------------------------------------------------------------------------------------
def box():
    f = np.full((96, 100), 1.0, np.float32)
    f[:, 30:35] = 2.0
    return f


case("flat_profile", "final", box, 40.0, 0.0, status=T.TOO_FAINT,
     note="a box at u = -10 .. -6 on a flat frame: significant in the refinement window, not in the profile window; peak = 0",
     half_width=16, wing=1, prof_half=2.0, prof_step=0.5, seg_len=32, n_iter=0)


def one_column():
    f = np.zeros((97, 100), np.float32)          # 96 valid positions: lower and upper median differ
    f[:, 40] = 1.0 + np.arange(97) / 1024.0     # distinct along the trail
    return f


case("fwhm_zero", "final", one_column, 40.0, 0.0, note="one bright column sampled at integer offsets: only the peak bin is >= peak/2",
     prop=lambda r, p: r["fwhm"] == 0.0 and r["fwhm_arcsec"] == 0.0 and r["peak"] > 1.0 and r["depth"] == 0.0,
     half_width=4, wing=1, prof_half=4.0, prof_step=1.0, seg_len=32, n_iter=1)

# ---- mask words --------------------------------------------------------------------------------------------------------------------
# (column centre, half-side, side of the trail the square lies on): the squares' column ranges [centre - half, centre + half)
MASK_OBJECTS = {
    100: [(4, 4, +1), (28, 4, -1), (36, 4, +1), (60, 4, -1), (68, 4, +1), (96, 4, -1)],
    333: [(4, 4, -1), (35, 4, +1), (29, 4, -1), (67, 4, +1), (61, 4, -1), (112, 17, -1), (311, 11, +1), (329, 4, -1)],
}
# the first and last column of every square, as the model test finds them in the oracle's mask
MASK_EDGES = {
    100: [(0, 7), (24, 31), (32, 39), (56, 63), (64, 71), (92, 99)],
    333: [(0, 7), (31, 38), (25, 32), (63, 70), (57, 64), (95, 128), (300, 321), (325, 332)],
}
MASK_SHAPES = {100: 96, 333: 200}


def mask_catalog(w, rho, theta, shift=0, margin=4):
    """a catalogue whose squares all reach `margin` rows across the line, alternately from either side; shift moves them along it"""
    h = MASK_SHAPES[w]
    th = float(np.float32(theta))
    objs = MASK_OBJECTS[w]
    n = len(objs)
    cat = {k: np.zeros((n, 5), np.float32) for k in ("ROWC", "COLC", "PSFMAG", "PETROTH90")}
    cat["PSFMAG"][:] = 15.0
    cat["NOBSERVE"] = np.ones(n, np.int32)
    cat["NDETECT"] = np.ones(n, np.int32)
    for i, (col, half, side) in enumerate(objs):
        col += shift
        y = (float(np.float32(rho)) - col * math.cos(th)) / math.sin(th)
        rt = int(round(h - 1 - y))                                  # the line's buffer row at the square's centre column
        row = rt + margin + 1 - half if side > 0 else rt - margin + half
        cat["ROWC"][i], cat["COLC"][i] = col, row                   # remove_stars reads rows from COLC and columns from ROWC
        cat["PETROTH90"][i] = 0 if half == 4 else half - 10
    return cat


def ramp_trail(h, w, seed, rho, theta):
    def make():
        y, x = np.mgrid[0:h, 0:w]
        f = ((0.001 * x + 0.00173205 * y).astype(np.float32) + noise(h, w, seed, 0.005) + gauss(h, w, rho, theta)).ravel()
        while True:                                 # every pixel its own value: the few repeated ones move up an ulp
            first = np.unique(f, return_index=True)[1]
            if len(first) == f.size:
                return f.reshape(h, w)
            again = np.setdiff1d(np.arange(f.size), first)
            f[again] = np.nextafter(f[again], np.float32(np.inf))
    return make


MASK = dict(half_width=8, wing=2, prof_half=6.0, prof_step=0.25, n_iter=2)
for _w, _L, _tilt in ((100, 20, 0.03), (333, 37, 0.02)):
    _h = MASK_SHAPES[_w]
    for _name, _th in ((f"mask_w{_w}", PI2), (f"mask_w{_w}_tilted", PI2 + _tilt)):
        _rho = centre_line(_h, _w, _th)
        case(_name, "mask", ramp_trail(_h, _w, _w + int(_th > PI2), _rho + 0.4, _th + 0.002), _rho, _th,
             cat=mask_catalog(_w, _rho, _th),
             note=f"w = {_w}: squares that start or end at columns 0, 31, 32, 63, 64 and w-1, some 8 px wide, on w = 333 one over "
                  "three words, all crossing the trail, on a frame of distinct values",
             prop=lambda r, p, n=_w // _L: 0 < r["min_valid"] < r["n_pos"] and r["n_seg"] == n, seg_len=_L, **MASK)
case("not_found_b", "mask", ramp_trail(96, 100, 99, 48.0, PI2), 48.0, PI2, status=T.NOT_FOUND, found=0,
     cat=mask_catalog(100, 48.0, PI2), note="a record without a detection, with a catalogue", seg_len=20, **MASK)


# ---- the restatement's results ----------------------------------------------------------------------------------------------------
def boxes_mask(c):
    """the case's star mask (boolean, buffer orientation) from the squares' definition (lfd_amd/csrc/k_image.h: k_rs_boxes),
    for catalogues like mask_catalog's: every object passes the tests and no slice bound is negative"""
    f = frame(c["name"])
    if c["cat"] is None:
        return None
    m = np.zeros(f.shape, bool)
    for i in range(len(c["cat"]["NOBSERVE"])):
        x, y = int(math.ceil(c["cat"]["COLC"][i, 2])), int(math.ceil(c["cat"]["ROWC"][i, 2]))
        pet = int(math.ceil(c["cat"]["PETROTH90"][i, 2]))
        d = int(pet / RS["pixscale"]) + 10 if pet > 0 else RS["defaultxy"]
        assert x - d >= 0 and y - d >= 0 and d <= RS["maxxy"]
        m[x - d:x + d, y - d:y + d] = True
    return m


_RESTATED = {}
_PRISTINE = {k: getattr(T, k) for k in ("lowmed", "sample", "positions", "n_segments", "wing_values", "longest_run", "medians",
                                        "_segment", "measure", "calc_fwhm", "depth")}


def restated(name, mask=None):
    """(record, profile) of the restatement for a named case: computed once, shared, never changed.  `mask` is the star mask
    the caller obtained (the oracle's, the library's): it has to equal the squares' definition, which is what is used."""
    c = CASES[name]
    want = boxes_mask(c)
    if mask is not None or want is not None:
        assert mask is not None and np.array_equal(mask, want), f"{name}: the star mask is not the catalogue's squares"
    if name not in _RESTATED:
        assert all(getattr(T, k) is v for k, v in _PRISTINE.items()), "the shared results come from the unpatched restatement only"
        _RESTATED[name] = T.measure(frame(name), c["rho"], c["theta"], found=c["found"], star_mask=want, **c["params"])
    return _RESTATED[name]
