"""Named frame seeing cases with hand-made finder records, built deterministically (include/lfdmi.h: frame seeing).

The finder never writes more than a handful of records into a test frame, never a NaN ``s_peak`` and never a flag beyond its
two bits, so the branches of k_psf_measure and k_psf_pack (lfd_amd/csrc/psf/k_psf.h) that only long lists, frame edges and odd
bit patterns reach need records written by hand.  A case is frames, records, frame records, sigma and parameters, and what it
is meant to hold: the status of every specially placed record and n_ok / n_packed / n_used per frame, worked out here from the
definition and never from tests/psf_ref.py.  tests/test_psf_cases_model.py holds the cases to that on the CPU,
tests/test_gpu_psf_edges.py runs them on the device.  Nothing here touches the device.

Record slots past a frame's n_out are garbage that would show if read: odd slots x = y = 2^31 - 1 with flags = -1, even slots a
clean candidate on top of one of the frame's own records (it would crowd that record), or in the frame's middle where the frame
has none (it would be counted)."""
import functools

import numpy as np

import psf_ref as R
import stars_ref as S

F32 = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
OK, NC, CLIPPED, CROWDED, BAD = R.OK, R.NOT_CANDIDATE, R.CLIPPED, R.CROWDED, R.BAD_PIXEL
SMALL = dict(win=1, gap=0, ring=1, iso=1)                   # H = 2: a 5 x 5 square, 16 ring pixels
PEAK = F32(1000.0)                                          # far above every floor


def from_bits(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


def bits_of(v):
    return int(np.asarray(v, np.float32).view(np.uint32))


def noise(shape, seed, scale=0.025):
    """seeded normal noise, float32, nowhere zero"""
    x = np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32)
    x[x == 0] = F32(2.0 ** -20)
    return x


def blank_records(n, max_obj):
    return np.zeros((n, max_obj), S.STAR_DTYPE)


def put(rec, f, i, x, y, rad=2, flags=0, s_peak=PEAK):
    rec[f, i] = (x, y, rad, flags, s_peak, 1.0, float(min(max(x, -1e6), 1e6)), float(min(max(y, -1e6), 1e6)))


def finish(frames, rec, n_out):
    """the garbage past n_out, the frame records, and everything read-only"""
    n, max_obj = rec.shape
    h, w = frames.shape[1:]
    for f in range(n):
        for k in range(int(n_out[f]), max_obj):
            if k % 2:
                rec[f, k] = (INT_MAX, INT_MAX, INT_MAX, -1, np.nan, np.nan, np.nan, np.nan)
            elif n_out[f]:
                src = rec[f, k % int(n_out[f])]
                put(rec, f, k, int(src["x"]), int(src["y"]))
            else:
                put(rec, f, k, w // 2, h // 2)
    frec = np.zeros(n, S.FRAME_DTYPE)
    frec["n_found"] = frec["n_out"] = n_out
    for a in (frames, rec, frec):
        a.setflags(write=False)
    return frames, rec, frec


class Case:
    """frames float32 [n, h, w], records [n, max_obj], frame_records [n], sigma (None or one per frame), params.  status:
    {(frame, index): intended status} of the specially placed records (of every record where ``every`` is set); n_ok, n_packed,
    n_used: intended per frame (n_used None where the pixels are plain noise and the case is not about it)."""

    def __init__(self, name, frames, rec, frec, sigma, params, status, n_ok, n_used=None, every=False):
        self.name, self.frames, self.records, self.frame_records, self.sigma, self.params = name, frames, rec, frec, sigma, dict(params)
        self.status, self.n_ok, self.n_used, self.every = dict(status), list(n_ok), n_used, every
        mu = self.params.get("max_used", R.DEFAULTS["max_used"])
        self.n_packed = [min(v, mu) for v in self.n_ok]

    def __repr__(self):
        return self.name

    @property
    def n_out(self):
        return [int(v) for v in self.frame_records["n_out"]]

    @property
    def max_obj(self):
        return self.records.shape[1]

    def big_endian(self):
        """the same pixels in big-endian bytes"""
        return self.frames.astype(">f4")

    def with_params(self, name, **params):
        return Case(name, self.frames, self.records, self.frame_records, self.sigma, dict(self.params, **params), self.status, self.n_ok,
                    self.n_used, self.every)


# ---- long_lists: more than 64 and more than 256 records, max_obj no multiple of 4, very different n_out in one launch -------
LL_SHAPE, LL_MAX_OBJ, LL_N_OUT = (64, 96), 1101, (1101, 257, 0, 65, 600)
LL_PARAMS = dict(SMALL, rad_max=32, e_max=1.0, min_stars=1, max_used=1024)
LL_CUTS = {"long_lists": 1024, "long_lists_cut300": 300, "long_lists_cut1": 1}


def ll_lattice():
    """the centres whose 5 x 5 square lies in the frame, on the spacing-2 lattice: no two within iso = 1"""
    h, w = LL_SHAPE
    return [(x, y) for y in range(2, h - 2, 2) for x in range(2, w - 2, 2)]


def ll_not_candidate(i):
    """the sprinkling: record 0, at least five records of every wave of 64, in no wave the same lanes"""
    return i % 11 == 0 or i % 64 == 5


def ll_frames():
    """By the parity of (row, column): 0.5 where either is even, 2.0 where both are odd, times noise of 1 %.  Around a lattice
    centre the ring's mean is 0.5 and the window's four diagonal pixels stand 1.5 above it: Q0 = 6, Qxx = Qyy = 6, Qxy = 0 in
    units of 2^30, so every OK record is used."""
    h, w = LL_SHAPE
    yy, xx = np.mgrid[0:h, 0:w]
    level = np.where((yy % 2 == 1) & (xx % 2 == 1), 2.0, 0.5)
    return np.stack([(level * (1.0 + noise((h, w), 100 + f, 0.01))).astype(np.float32) for f in range(len(LL_N_OUT))])


@functools.lru_cache(maxsize=None)
def long_lists():
    frames = ll_frames()
    lattice = ll_lattice()
    assert len(lattice) == 1380
    rec = blank_records(len(LL_N_OUT), LL_MAX_OBJ)
    status, n_ok = {}, []
    for f, n in enumerate(LL_N_OUT):
        order = np.random.default_rng(200 + f).permutation(len(lattice))[:n]
        for i, k in enumerate(order):
            nc = ll_not_candidate(i)
            put(rec, f, i, *lattice[k], rad=1 + i % 32, flags=4 if nc else 0)
            status[(f, i)] = NC if nc else OK
        n_ok.append(sum(not ll_not_candidate(i) for i in range(n)))
    return Case("long_lists", *finish(frames, rec, LL_N_OUT), None, LL_PARAMS, status, n_ok, n_used="packed", every=True)


# ---- crowd_far: the only neighbour of a record in the second and third stride of the crowding loop --------------------------
CF_CELL, CF_COLS, CF_ROWS, CF_N, CF_MAX_OBJ = 30, 12, 10, 130, 133
CF_SHAPE = (12 + CF_CELL * (CF_ROWS - 1) + 13 + 13, 12 + CF_CELL * (CF_COLS - 1) + 13 + 13)      # 308 x 368
# (index, partner index, partner's offset, partner's flags, status of the record, status of the partner); iso = 12
CF_PAIRS = [(3, 64, (5, 3), 0, CROWDED, CROWDED),           # the only neighbour in the second stride
            (5, 129, (12, 7), 0, CROWDED, CROWDED),         # in the third, the last record of all
            (7, 70, (4, 4), S.EXTENDED, CROWDED, NC),       # a neighbour that is no candidate still crowds
            (8, 100, (0, 0), 0, CROWDED, CROWDED),          # the same position: d = 0
            (10, 65, (12, 0), 0, CROWDED, CROWDED), (11, 66, (13, 0), 0, OK, OK),       # iso and iso + 1 in x only
            (12, 67, (0, 12), 0, CROWDED, CROWDED), (13, 68, (0, 13), 0, OK, OK),       # in y only
            (14, 69, (12, 12), 0, CROWDED, CROWDED), (15, 71, (13, 13), 0, OK, OK)]     # on the diagonal


@functools.lru_cache(maxsize=None)
def crowd_far():
    """A site every 30 px: a pair's partner lies up to 13 px right of and below its site, 17 px from the next one."""
    frames = noise((1, *CF_SHAPE), 300)
    rec = blank_records(1, CF_MAX_OBJ)
    site = lambda k: (12 + CF_CELL * (k % CF_COLS), 12 + CF_CELL * (k // CF_COLS))           # noqa: E731
    status, taken = {}, set()
    for k, (i, j, (dx, dy), flags, st_i, st_j) in enumerate(CF_PAIRS):
        x, y = site(k)
        put(rec, 0, i, x, y)
        put(rec, 0, j, x + dx, y + dy, flags=flags)
        status[(0, i)], status[(0, j)] = st_i, st_j
        taken |= {i, j}
    k = len(CF_PAIRS)
    for i in range(CF_N):
        if i not in taken:
            put(rec, 0, i, *site(k))
            status[(0, i)] = OK
            k += 1
    assert k == CF_COLS * CF_ROWS
    n_ok = [sum(st == OK for st in status.values())]
    return Case("crowd_far", *finish(frames, rec, [CF_N]), None, {}, status, n_ok, every=True)


# ---- clip_all_sides: the four comparisons of the clip test, the last pixel of the last frame ----------------------------------
CLIP_SHAPE, CLIP_H = (40, 56), 12


@functools.lru_cache(maxsize=None)
def clip_all_sides():
    """Defaults but iso = 1 (H = 12): legal centres are x 12 .. 43, y 12 .. 27.  Frame 0 the x edges, frame 1 the y edges and
    two records far outside, the last frame the four legal corners: the square of (43, 27) ends on the buffer's last pixel."""
    h, w = CLIP_SHAPE
    H = CLIP_H
    frames = noise((3, h, w), 400)
    rec = blank_records(3, 7)
    recs = {0: [((H - 1, 14), CLIPPED), ((H, 17), OK), ((w - 1 - H, 20), OK), ((w - H, 23), CLIPPED)],
            1: [((20, H - 1), CLIPPED), ((24, H), OK), ((28, h - 1 - H), OK), ((32, h - H), CLIPPED), ((INT_MIN, 20), CLIPPED),
                ((36, INT_MAX), CLIPPED)],
            2: [((H, H), OK), ((w - 1 - H, H), OK), ((H, h - 1 - H), OK), ((w - H, 20), CLIPPED), ((30, h - H), CLIPPED),
                ((w - 1 - H, h - 1 - H), OK)]}
    status = {}
    for f, lst in recs.items():
        for i, ((x, y), st) in enumerate(lst):
            put(rec, f, i, x, y)
            status[(f, i)] = st
    n_out = [len(recs[f]) for f in range(3)]
    n_ok = [sum(st == OK for (g, _), st in status.items() if g == f) for f in range(3)]
    return Case("clip_all_sides", *finish(frames, rec, n_out), None, dict(iso=1, min_stars=1), status, n_ok, every=True)


@functools.lru_cache(maxsize=None)
def clip_25():
    """A frame of exactly (2 H + 1)^2: (12, 12) is the only legal centre.  Frames 0 - 3 hold one of its four neighbours each,
    frame 4 all five (the neighbours are clipped and still crowd the centre), the last frame the centre alone."""
    frames = noise((6, 25, 25), 410)
    rec = blank_records(6, 6)
    around = [(11, 12), (13, 12), (12, 11), (12, 13)]
    status = {}
    for f, (x, y) in enumerate(around):
        put(rec, f, 0, x, y)
        status[(f, 0)] = CLIPPED
    for i, (x, y) in enumerate([(12, 12)] + around):
        put(rec, 4, i, x, y)
        status[(4, i)] = CLIPPED if i else CROWDED
    put(rec, 5, 0, 12, 12)
    status[(5, 0)] = OK
    return Case("clip_25", *finish(frames, rec, [1, 1, 1, 1, 5, 1]), None, dict(iso=1, min_stars=1), status, [0, 0, 0, 0, 0, 1], every=True)


# ---- 5 x 5 patches: one record per patch ---------------------------------------------------------------------------------------

def patch_centre(k, cols):
    return 2 + 5 * (k % cols), 2 + 5 * (k // cols)


def plain_star(frame, cx, cy, rng):
    """An ordinary small star, 1 % noise on each level: 1 at the peak, 1/4 on the arms, 1/16 in the window's corners, 1/32 in
    the ring.  Q0, Qxx and Qyy are positive and stay so when one pixel is replaced by a value below 1/4: the star is used."""
    base = np.full((5, 5), 0.03125)
    base[1:4, 1:4] = 0.0625
    base[2, 1:4] = base[1:4, 2] = 0.25
    base[2, 2] = 1.0
    frame[cy - 2:cy + 3, cx - 2:cx + 3] = (base * (1.0 + 0.01 * rng.standard_normal((5, 5)))).astype(np.float32)


WINDOW_AT, RING_AT = (1, -1), (2, 1)                        # (dx, dy) of the special pixel: a window corner, a ring pixel
CORNERS = [(-1, -1), (1, -1), (-1, 1), (1, 1)]
RING = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if max(abs(dx), abs(dy)) == 2]


def fix_named_patterns():
    """the issue's list, positive; every one is used in both signs"""
    ties = [bits_of(F32(k * 2.0 ** -31)) for k in (1, 3, 5, 7)]             # v 2^30 = 0.5, 1.5, 2.5, 3.5
    return ties + [0x2fffffff,                              # just under 0.5
                   0x2f800000, 0x2f7fffff, 0x2f000000, 0x20000000,          # 2^-32 (sh = -25) and below (the q = 0 branch)
                   0x00000001, 0x007fffff, 0x00800000,      # the smallest and the largest denormal, the smallest normal
                   0x33000001, 0x33000000,                  # 32 + 2^-18 and 32
                   0x30000001, 0x307fffff, 0x30800000,      # just over 0.5, just under 1, 1
                   0x3b800001, 0x3bffffff, 0x3c000000, 0x3c000001]          # s = 1 (one bit shifted out) and sh = 0


def fix_tie_patterns():
    """Every shift s = 1 .. 25 of psf_fix (exponent 120 - s): mantissas m with m / 2^s on a tie above an even and above an odd
    integer, and one unit of m to either side."""
    out = []
    for s in range(1, 26):
        half, base = 1 << (s - 1), (1 << 23) >> s
        for u in (base, base + 1):
            for m in ((u << s) | half, ((u << s) | half) - 1, ((u << s) | half) + 1):
                if (1 << 23) <= m < (1 << 24):
                    out.append(((120 - s) << 23) | (m & 0x7fffff))
    return sorted(set(out))


FIX_COLS = 12


@functools.lru_cache(maxsize=None)
def fix_edges():
    """One star per named pattern, sign and place (a window corner; a ring pixel) with ordinary pixels around it; stars whose
    four window corners and sixteen ring pixels are all tie patterns of alternating sign; a ring of -3 and one -4 (Q_ring = -49,
    b = -3 as C divides); a window below its ring (Q0 < 0) and one level with it (Q0 = 0): packed, not used."""
    named = [p | sgn for p in fix_named_patterns() for sgn in (0, 0x80000000)]
    ties = fix_tie_patterns()
    ties = [p | (0x80000000 if k % 2 else 0) for k, p in enumerate(ties)]
    n_dense = -(-len(ties) // 20)
    n = 2 * len(named) + n_dense + 3
    rows = -(-n // FIX_COLS)
    rng = np.random.default_rng(500)
    frame = np.zeros((5 * rows, 5 * FIX_COLS), np.float32)
    for k in range(rows * FIX_COLS):
        plain_star(frame, *patch_centre(k, FIX_COLS), rng)
    rec = blank_records(1, n + 3)
    special = {}                                            # record -> [(y, x, bits)]
    k = 0
    for p in named:
        for dx, dy in (WINDOW_AT, RING_AT):
            cx, cy = patch_centre(k, FIX_COLS)
            special[k] = [(cy + dy, cx + dx, p)]
            k += 1
    for d in range(n_dense):
        cx, cy = patch_centre(k, FIX_COLS)
        mine = [ties[(20 * d + j) % len(ties)] for j in range(20)]
        special[k] = [(cy + dy, cx + dx, b) for (dx, dy), b in zip(CORNERS + RING, mine)]
        k += 1
    cx, cy = patch_centre(k, FIX_COLS)
    three, four = bits_of(F32(-3 * 2.0 ** -30)), bits_of(F32(-4 * 2.0 ** -30))
    special[k] = [(cy + dy, cx + dx, four if j == 0 else three) for j, (dx, dy) in enumerate(RING)]
    k += 1
    unused = []
    for ring_level in (0.5, 0.25):
        cx, cy = patch_centre(k, FIX_COLS)
        frame[cy - 2:cy + 3, cx - 2:cx + 3] = ring_level
        frame[cy - 1:cy + 2, cx - 1:cx + 2] = 0.25
        special[k] = []
        unused.append(k)
        k += 1
    assert k == n
    for i, px in special.items():
        put(rec, 0, i, *patch_centre(i, FIX_COLS))
        for y, x, b in px:
            frame[y, x] = from_bits(b)[0]
    frames = frame[None]
    assert not (frames == 0).any()
    c = Case("fix_edges", *finish(frames, rec, [n]), None, dict(SMALL, e_max=1.0, min_stars=1, max_used=1024),
             {(0, i): OK for i in range(n)}, [n], n_used=[n - 2], every=True)
    c.special, c.unused, c.patterns = special, unused, sorted(set(named) | set(ties) | {three, four})
    return c


# ---- sat_edges: |v| <= (float)sat --------------------------------------------------------------------------------------------
SAT_COLS = 6
SATS = {"sat_20": 20.0, "sat_20_1": 20.1, "sat_default": R.MAX_SAT}


def sat_values():
    out = []
    for s in (20.0, 20.1, 4096.0):
        f = F32(s)
        out += [np.nextafter(f, F32(0)), f, np.nextafter(f, F32(np.inf))]
    return out


@functools.lru_cache(maxsize=None)
def sat_frame():
    """One star per value (each of 20, (float)20.1 and 4096, one ulp below and one above), sign and place: the window's centre
    or a ring pixel.  (float)20.1 lies above 20.1, so a comparison in double would refuse it."""
    vals = [F32(sg) * v for v in sat_values() for sg in (1, -1)]
    n = 2 * len(vals)
    assert n == SAT_COLS * SAT_COLS
    rng = np.random.default_rng(600)
    frame = np.zeros((5 * SAT_COLS, 5 * SAT_COLS), np.float32)
    rec = blank_records(1, n + 2)
    placed = []
    for k in range(n):
        cx, cy = patch_centre(k, SAT_COLS)
        plain_star(frame, cx, cy, rng)
        v, in_ring = vals[k // 2], bool(k % 2)
        dx, dy = RING_AT if in_ring else (0, 0)
        frame[cy + dy, cx + dx] = v
        put(rec, 0, k, cx, cy)
        placed.append((F32(v), in_ring))
    return finish(frame[None], rec, [n]), placed


@functools.lru_cache(maxsize=None)
def sat_edges(name):
    """A star is OK when its value is within (float)sat.  It is used when the value lifts the window over the ring: at the
    centre and positive, or in the ring and negative (the ring's mean drops below every window pixel)."""
    (frames, rec, frec), placed = sat_frame()
    lim = F32(SATS[name])
    status = {(0, k): OK if abs(v) <= lim else BAD for k, (v, _) in enumerate(placed)}
    used = sum(status[(0, k)] == OK and ((v > 0) != in_ring) for k, (v, in_ring) in enumerate(placed))
    c = Case(name, frames, rec, frec, None, dict(SMALL, sat=SATS[name], e_max=1.0, min_stars=1), status,
             [sum(st == OK for st in status.values())], n_used=[used], every=True)
    c.patterns = sorted({bits_of(v) for v, _ in placed})
    return c


# ---- extremes: the largest sums the parameters allow -------------------------------------------------------------------------
EXT_PARAMS = dict(win=16, gap=8, ring=8, iso=1, rad_max=32, e_max=1.0, min_stars=1)     # H = 32: a 65 x 65 square
EXT_H = 32
# name -> (the window's sign as a function of (dx, dy), the ring's sign, used).  p = q - b is 2^43 where the window's sign
# differs from the ring's and 0 elsewhere; Q0 > 0 wants the ring negative, and then the pixels at 2^43 fill a half plane or
# two quadrants, whose second moments about their mean are positive.
EXT_KINDS = {"up": (lambda dx, dy: 1, -1, True), "down": (lambda dx, dy: -1, 1, False),
             "qx": (lambda dx, dy: 1 if dx >= 0 else -1, -1, True), "qx_neg": (lambda dx, dy: -1 if dx >= 0 else 1, 1, False),
             "qy": (lambda dx, dy: 1 if dy >= 0 else -1, -1, True), "qy_neg": (lambda dx, dy: -1 if dy >= 0 else 1, 1, False),
             "qxy": (lambda dx, dy: 1 if dx * dy >= 0 else -1, -1, True), "qxy_neg": (lambda dx, dy: -1 if dx * dy > 0 else 1, -1, True)}
EXT_LAYOUT = {"extremes_65": ((65, 65), [("up", 32, 32), ("down", 32, 32), ("qx", 32, 32), ("qx_neg", 32, 32), ("qy", 32, 32),
                                         ("qy_neg", 32, 32), ("qxy", 32, 32), ("qxy_neg", 32, 32)]),
              "extremes_70x80": ((70, 80), [("down", 32, 32), ("qxy", 40, 35), ("qx_neg", 47, 32), ("qy", 32, 37), ("up", 47, 37)])}
EXT_QXX_UP = 868491040640729088                             # 2^43 * 33 * 2992: sixty bits


def ext_frame(shape, kind, cx, cy, seed):
    """+-4096 in the window and the ring as the kind says, +-4096 by a seeded coin in the gap, noise elsewhere"""
    sign, ring_sign, _ = EXT_KINDS[kind]
    f = noise(shape, seed)
    coin = np.random.default_rng(seed).integers(0, 2, (65, 65)) * 2 - 1
    for dy in range(-EXT_H, EXT_H + 1):
        for dx in range(-EXT_H, EXT_H + 1):
            d = max(abs(dx), abs(dy))
            s = sign(dx, dy) if d <= 16 else ring_sign if d > 24 else coin[dy + EXT_H, dx + EXT_H]
            f[cy + dy, cx + dx] = F32(4096.0 * s)
    return f


@functools.lru_cache(maxsize=None)
def extremes(name):
    """One record per frame; the last frame of the 70 x 80 batch holds the bottom-right legal centre."""
    shape, layout = EXT_LAYOUT[name]
    frames = np.stack([ext_frame(shape, kind, cx, cy, 700 + k) for k, (kind, cx, cy) in enumerate(layout)])
    rec = blank_records(len(layout), 3)
    for f, (kind, cx, cy) in enumerate(layout):
        put(rec, f, 0, cx, cy, rad=32)
    c = Case(name, *finish(frames, rec, [1] * len(layout)), None, EXT_PARAMS, {(f, 0): OK for f in range(len(layout))},
             [1] * len(layout), n_used=[int(EXT_KINDS[kind][2]) for kind, _, _ in layout], every=True)
    c.layout = layout
    c.patterns = [bits_of(F32(4096.0)), bits_of(F32(-4096.0))]
    return c


# ---- candidate_edges: records the finder cannot write ---------------------------------------------------------------------------
CAND_SIGMA = (0.025, 0.4, 0.0125)
CAND_PARAMS = dict(SMALL, k_peak=33.3, rad_max=16, e_max=1.0, min_stars=1)
CAND_COLS = 6


def cand_floor(sigma):
    """(float)(k_peak * 3.0 * (double)sigma)"""
    return F32(CAND_PARAMS["k_peak"] * 3.0 * float(F32(sigma)))


@functools.lru_cache(maxsize=None)
def candidate_edges():
    """Three frames with three sigmas, the same records in each: every frame's floor and the float below it as s_peak (a
    candidate in the frames whose floor is not above it), NaN and the infinities; the radii and the flags one field at a time."""
    floors = [cand_floor(s) for s in CAND_SIGMA]
    peaks = [v for fl in floors for v in (fl, np.nextafter(fl, F32(0)))] + [F32(np.nan), F32(np.inf), F32(-np.inf), F32(0.0)]
    rads = [(0, NC), (1, OK), (16, OK), (17, NC), (-1, OK), (INT_MIN, OK), (INT_MAX, NC)]
    flags = [(0, OK), (S.EXTENDED, NC), (S.EDGE, NC), (4, NC), (INT_MIN, NC), (3, NC), (-1, NC)]
    n = len(peaks) + len(rads) + len(flags)
    rows = -(-n // CAND_COLS)
    rng = np.random.default_rng(800)
    frames = np.zeros((3, 5 * rows, 5 * CAND_COLS), np.float32)
    rec = blank_records(3, n + 1)
    status = {}
    for f in range(3):
        for k in range(rows * CAND_COLS):
            plain_star(frames[f], *patch_centre(k, CAND_COLS), rng)
        for k in range(n):
            xy = patch_centre(k, CAND_COLS)
            if k < len(peaks):
                put(rec, f, k, *xy, s_peak=peaks[k])
                status[(f, k)] = OK if peaks[k] >= floors[f] else NC        # (NaN compares false)
            elif k < len(peaks) + len(rads):
                rad, st = rads[k - len(peaks)]
                put(rec, f, k, *xy, rad=rad)
                status[(f, k)] = st
            else:
                fl, st = flags[k - len(peaks) - len(rads)]
                put(rec, f, k, *xy, flags=fl)
                status[(f, k)] = st
    n_ok = [sum(st == OK for (g, _), st in status.items() if g == f) for f in range(3)]
    c = Case("candidate_edges", *finish(frames, rec, [n] * 3), np.array(CAND_SIGMA, np.float32), CAND_PARAMS, status, n_ok,
             n_used="packed", every=True)
    c.floors, c.n_peaks = floors, len(peaks)
    return c


# ---- the cases by name ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def get(name):
    if name in LL_CUTS:
        base = long_lists()
        return base if name == "long_lists" else base.with_params(name, max_used=LL_CUTS[name])
    if name in SATS:
        return sat_edges(name)
    if name in EXT_LAYOUT:
        return extremes(name)
    return {"crowd_far": crowd_far, "clip_all_sides": clip_all_sides, "clip_25": clip_25, "fix_edges": fix_edges,
            "candidate_edges": candidate_edges}[name]()


NAMES = tuple(LL_CUTS) + ("crowd_far", "clip_all_sides", "clip_25", "fix_edges") + tuple(SATS) + tuple(EXT_LAYOUT) + ("candidate_edges",)
DEVICE_ROUTE = tuple(LL_CUTS) + ("crowd_far", "clip_all_sides", "clip_25")          # device frames with device records
BIG_ENDIAN = ("fix_edges", "clip_all_sides", "clip_25")


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement's answer for a case, computed once and left unchanged: (packed, frame records)"""
    c = get(name)
    out = R.measure_batch(c.frames, c.records, c.frame_records, c.sigma, **c.params)
    for a in out:
        a.setflags(write=False)
    return out


NOT_REACHED = {
    "the 65th column in lane 0 with a clipped neighbour": "win = 16, gap = 8, ring = 8 is the only 65-wide square; extremes runs it at both frame shapes",
    "sums beyond 2^62": "the header's bound: |q - b| <= 2^43 times dx^2 <= 2^8 times 33^2 < 2^11 pixels; extremes reaches 60 bits, the most the parameters allow",
    "n_out above max_obj or below 0": "refused by the host (LFDMI_ERR_ARG) before a kernel runs; tests/test_gpu_psf.py",
}
