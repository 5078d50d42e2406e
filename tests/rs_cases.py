"""Named remove_stars cases, a literal restatement of the reference and a plain restatement of which route the host takes.

remove_stars blots a square per selected catalogue object: ``img[x-d:x+d, y-d:y+d].fill(0.0)`` with x = ceil(COLC) on axis 0 and
real Python slices, so a centre with ``x + d < 0`` wraps to the far edge.  The library applies the squares in three ways (the
mask in the bright sweep of lfdmi_detect_batch, the zero fill object by object, the sorted squares blotted band by band) and the
host picks among them in enqueue_detect_front / run_removestars / rs_fill_point (lfdmi.hip).  ``literal`` is the reference,
``squares`` the same slices as index ranges, ``route`` the host's choice.  Nothing here touches the device:
tests/test_rs_cases_model.py checks the cases on the CPU, tests/test_gpu_rs_routes.py runs them on the device.

Frames are a flat level with a slow ramp in both directions (non-zero everywhere after prep, so GRAY is zero exactly on the
blotted pixels and a row / column mix-up shows).  ``Case.frame`` is what the caller passes, in the catalogue's orientation; the
passes see it flipped (``frame[::-1]``)."""
import math

import numpy as np

import front_cases as fc

# ---- constants of the kernels (k_image.h) and of the host (lfdmi.hip) -------------------------------------------------------
RS_MAXW, RS_MAXROWS, RS_BAND_ROWS, RS_SORT_MIN, RS_SORT_MAXH = 4096, 16, 8, 1024, 8192
WORD, NIBBLE, FILL_LANES, SORT_THREADS = 32, 4, 64, 1024
FILL_POINTS = (1, 2, 3, 4, 5, 12, 13, 14, 15)   # rs_fill_point(k) in the order a delta chunk visits them; then -1
MAX_PIXELS = 300_000
FILTERS = "ugriz"
CAPS = {'u': 22.0, 'g': 22.2, 'r': 22.2, 'i': 21.3, 'z': 20.5}
RS_DEFAULT = dict(defaultxy=6, maxxy=25, pixscale=0.396, magcount=3, maxmagdiff=3, filter_caps=CAPS)
ERODE_1x1 = fc.ONES(1, 1)                       # the dim pass of the device tests: ERODED == EQUALIZED, the mask pixel by pixel


# ---- the reference ----------------------------------------------------------------------------------------------------------

def _selected(cat, i, filter, defaultxy, filter_caps, maxxy, pixscale, magcount, maxmagdiff):
    """The catalogue tests of one object: (x, y, dxy) of its square, or None where the object stays."""
    fi = FILTERS.index(filter)
    x = int(math.ceil(cat["COLC"][i][fi]))
    y = int(math.ceil(cat["ROWC"][i][fi]))
    mags = [math.ceil(v) for v in cat["PSFMAG"][i]]
    if not mags[fi] < filter_caps[filter]:
        return None
    diffs = np.absolute([mags[j] - mags[k] for j in range(5) for k in range(j + 1, 5)])
    if not magcount >= np.count_nonzero(diffs > maxmagdiff):
        return None
    dxy = defaultxy
    pet = math.ceil(cat["PETROTH90"][i][fi])
    if pet > 0:
        dxy = int(pet / pixscale) + 10
    if dxy > maxxy:
        dxy = defaultxy
    if cat["NOBSERVE"][i] != cat["NDETECT"][i]:
        return None
    return x, y, dxy


def literal(img, cat, filter, **rs):
    """A blotted copy of ``img``: the reference's loop with real numpy slices."""
    out = np.array(img, np.float32, copy=True)
    kw = dict(RS_DEFAULT, **rs)
    for i in range(0 if cat is None else len(cat["NOBSERVE"])):
        s = _selected(cat, i, filter, **kw)
        if s is not None:
            x, y, dxy = s
            out[x - dxy:x + dxy, y - dxy:y + dxy].fill(0.0)
    return out


def squares(cat, filter, shape, **rs):
    """Per object: None where it stays, else its slices as (r0, r1, c0, c1) (r1 <= r0 or c1 <= c0: nothing blotted)."""
    kw = dict(RS_DEFAULT, **rs)
    out = []
    for i in range(0 if cat is None else len(cat["NOBSERVE"])):
        s = _selected(cat, i, filter, **kw)
        if s is None:
            out.append(None)
            continue
        x, y, dxy = s
        r0, r1, _ = slice(x - dxy, x + dxy).indices(shape[0])
        c0, c1, _ = slice(y - dxy, y + dxy).indices(shape[1])
        out.append((r0, r1, c0, c1))
    return out


def is_empty(sq):
    return sq[1] <= sq[0] or sq[3] <= sq[2]


def wrapped(cat, filter, **rs):
    """True where a selected object's slice stops below zero on either axis (the wrap to the far edge)."""
    kw = dict(RS_DEFAULT, **rs)
    for i in range(len(cat["NOBSERVE"])):
        s = _selected(cat, i, filter, **kw)
        if s is not None and (s[0] + s[2] < 0 or s[1] + s[2] < 0):
            return True
    return False


# ---- the host's choice ------------------------------------------------------------------------------------------------------

def dim_params(erode=ERODE_1x1):
    pb, pd = fc.default_params()
    return dict(pb, lwTresh=1e9), dict(pd, erodeKernel=erode)


def route(h, w, n_obj, loc, cat_loc, dtype, knobs, dim_par, mode=0):
    """What lfdmi_detect_batch does with the squares of a chunk.  loc: "device" / "host" / "pinned"; cat_loc: "host" / "device";
    dtype: "f32" / "be"; n_obj: the catalogue's max_obj (0: no catalogue); mode: lfdmi_set_stage_images.  Returns a dict:
    delta   the dim pass rebuilds its image from the bright sweep's bit planes (front_cases.route: front == "bits")
    fold    the sweep masks the squares (k_prep_hist<1, true, ., RS>), else they are zero-filled in front of it
    sorted  k_rs_sort + rs_mark / k_rs_fill_bands, else per object (the loop in the sweep, k_rs_fill)
    side    the deferred fill of device frames: None, "bands", "one" launch or "two" (halves at LFDMI_RS_FILL_AT0 and _AT)
    back    how the caller's frames end up blotted: "filled" (in place on the device), "host blot" (host threads with the squares
            copied back), "copy back" (the device copy travels back), "untouched" (big-endian frames)."""
    knobs = knobs or {}
    iv = lambda k, d: int(knobs.get(k, d))                                           # noqa: E731
    delta = fc.route(h, w, dim_par, "batch", mode, knobs)["front"] == "bits"
    on_host, be = loc != "device", dtype == "be"
    host_blot = n_obj > 0 and on_host and cat_loc == "host" and not be
    copy_back = n_obj > 0 and on_host and not host_blot and not be
    fold = bool(n_obj > 0 and iv("LFDMI_RS_FOLD", 1) and delta and w <= RS_MAXW and not copy_back)
    srt = bool(n_obj > iv("LFDMI_RS_SORT_MIN", RS_SORT_MIN) and h < RS_SORT_MAXH and w % WORD == 0 and w <= RS_MAXW)
    side = None
    if fold and not on_host:
        at0, at = iv("LFDMI_RS_FILL_AT0", 3), iv("LFDMI_RS_FILL_AT", 13)
        first = at0 in FILL_POINTS and (at not in FILL_POINTS or FILL_POINTS.index(at0) <= FILL_POINTS.index(at))
        side = "bands" if srt else ("two" if first else "one")
    back = "none" if n_obj <= 0 else "untouched" if (be and on_host) else "host blot" if host_blot else "copy back" if copy_back else "filled"
    return dict(delta=delta, fold=fold, sorted=srt, side=side, back=back)


def fill_halves(max_obj, frac=0.5):
    """rs_fill_point's split of the k_rs_fill blocks (four objects each): (blocks in the first part, blocks in all)."""
    nblk = (max_obj + 3) // 4
    return max(0, min(nblk, int(nblk * frac))), nblk


def sort_rows_per_thread(h):
    return (h + 1 + SORT_THREADS - 1) // SORT_THREADS


def hmax(**rs):
    kw = dict(RS_DEFAULT, **rs)
    return 2 * max(kw["maxxy"], kw["defaultxy"])


# ---- frames and catalogues --------------------------------------------------------------------------------------------------

def flat(h, w):
    """40 and a little more: a ramp of 12 levels down the rows and 18 along the columns (thirty levels: after the equalisation
    no step between neighbours is high enough for Canny), float32, nowhere zero after prep."""
    yy, xx = np.mgrid[0:h, 0:w]
    # (clipped at both ends: the lowest level is populous, so the equalisation maps it above zero and only blotted pixels are 0)
    return (40.25 + np.clip(12.0 * yy / max(h, 2) + 18.0 * xx / max(w, 2), 4.0, 26.0)).astype(np.float32)


def O(x, y, d=None, pet=0.0, mags=15.0, nobs=1, ndet=1):                              # noqa: E743
    """One object: x the centre on axis 0 (COLC), y on axis 1 (ROWC), scalars or one value per filter.  d: a Petrosian size that
    gives dxy == d where the case's pixscale is 1 (d >= 11)."""
    if d is not None:
        assert d >= 11
        pet = float(d - 10)
    return dict(x=x, y=y, pet=pet, mags=mags, nobs=nobs, ndet=ndet)


def catalogue(objs):
    n = len(objs)
    five = lambda v: np.broadcast_to(np.asarray(v, np.float32), (5,))                # noqa: E731
    cat = {"COLC": np.zeros((n, 5), np.float32), "ROWC": np.zeros((n, 5), np.float32), "PSFMAG": np.zeros((n, 5), np.float32),
           "PETROTH90": np.zeros((n, 5), np.float32), "NOBSERVE": np.zeros(n, np.int32), "NDETECT": np.zeros(n, np.int32)}
    for i, o in enumerate(objs):
        cat["COLC"][i], cat["ROWC"][i], cat["PSFMAG"][i], cat["PETROTH90"][i] = five(o["x"]), five(o["y"]), five(o["mags"]), five(o["pet"])
        cat["NOBSERVE"][i], cat["NDETECT"][i] = o["nobs"], o["ndet"]
    for v in cat.values():
        v.setflags(write=False)
    return cat


class Case:
    """One frame, one catalogue, one parameter set.  named: {object index: (r0, r1, c0, c1) | "empty" | None (the object stays)},
    worked out by hand where the case is defined.  seams: ("row" | "col", index) in the caller's orientation: blotted and kept
    pixels lie within 2 px of it.  nothing: no pixel is blotted at all.  batch: the case also goes through lfdmi_detect_batch.
    expect: route fields for device frames, a host catalogue, stage images off."""

    def __init__(self, name, row, h, w, objs, rs=None, filter="r", knobs=None, named=None, seams=(), expect=None, nothing=False, batch=True):
        self.name, self.row, self.h, self.w, self.objs, self.filter = name, row, h, w, list(objs), filter
        self.rs, self.knobs, self.named, self.seams = dict(rs or {}), dict(knobs or {}), dict(named or {}), tuple(seams)
        self.expect, self.nothing, self.batch = dict(expect or {}), nothing, batch
        self._frame = self._cat = self._lit = None
        assert h * w <= MAX_PIXELS, name

    def __repr__(self):
        return self.name

    @property
    def frame(self):
        if self._frame is None:
            self._frame = flat(self.h, self.w)
            self._frame.setflags(write=False)
        return self._frame

    @property
    def cat(self):
        if self._cat is None:
            self._cat = catalogue(self.objs)
        return self._cat

    @property
    def kw(self):
        return dict(RS_DEFAULT, **self.rs)

    @property
    def literal(self):
        if self._lit is None:
            self._lit = literal(self.frame, self.cat, self.filter, **self.rs)
            self._lit.setflags(write=False)
        return self._lit

    def squares(self):
        return squares(self.cat, self.filter, (self.h, self.w), **self.rs)


CASES = []


def case(*a, **k):
    CASES.append(Case(*a, **k))


SIZES = dict(pixscale=1.0)                      # dxy = PETROTH90 + 10: any size from 11 up to maxxy, the default below that

# -- Python slices (d = 6 on 40 x 160) ----------------------------------------------------------------------------------------
SL = "python slices"
case("wrap_rows", SL, 40, 160, [O(-8, 20), O(-7, 50), O(-40, 80), O(-41, 110), O(-46, 140)],
     named={0: (26, 38, 14, 26), 1: (27, 39, 44, 56), 2: (0, 6, 74, 86), 3: (0, 5, 104, 116), 4: "empty"},
     seams=[("row", 26), ("row", 38), ("row", 39), ("row", 6), ("row", 5)], expect=dict(delta=True, fold=True, sorted=False, side="two"))
case("wrap_cols", SL, 40, 160, [O(20, -8), O(10, -7), O(30, -160), O(8, -161), O(20, -166)],
     named={0: (14, 26, 146, 158), 1: (4, 16, 147, 159), 2: (24, 36, 0, 6), 3: (2, 14, 0, 5), 4: "empty"},
     seams=[("col", 146), ("col", 158), ("col", 159), ("col", 6), ("col", 5)])
case("slice_empty", SL, 40, 160, [O(-3, 40), O(20, -3), O(0, 80), O(-6, 100), O(47, 40), O(46, 60), O(20, 167), O(20, 166)],
     named={i: "empty" for i in range(8)}, nothing=True)
case("slice_exact", SL, 40, 160, [O(6, 20), O(34, 50), O(40, 80), O(45, 110), O(20, 6), O(20, 154), O(33, 160), O(8, 165)],
     named={0: (0, 12, 14, 26), 1: (28, 40, 44, 56), 2: (34, 40, 74, 86), 3: (39, 40, 104, 116), 4: (14, 26, 0, 12), 5: (14, 26, 148, 160),
            6: (27, 39, 154, 160), 7: (2, 14, 159, 160)},
     seams=[("row", 12), ("row", 28), ("row", 34), ("row", 39), ("col", 12), ("col", 148), ("col", 154), ("col", 159)])
case("short_h_lt_d", SL, 17, 96, [O(20, 30), O(10, 70), O(-22, 93)], rs=dict(defaultxy=20),
     named={0: (0, 17, 10, 50), 1: (7, 17, 50, 90), 2: (0, 15, 73, 96)}, seams=[("row", 7), ("row", 15), ("col", 10)])
case("short_h_lt_2d", SL, 33, 96, [O(20, 30), O(25, 75), O(10, 75)], rs=dict(defaultxy=20),
     named={0: (0, 33, 10, 50), 1: (5, 33, 55, 95), 2: (23, 30, 55, 95)}, seams=[("row", 5), ("col", 50), ("col", 55), ("col", 95)])
case("cover_all", SL, 36, 32, [O(20, 20)], rs=dict(defaultxy=20), named={0: (0, 36, 0, 32)})

# -- the 32-bit word of the mask, the nibble of the band fill (100 x 160: five words) --------------------------------------------
WORDS = "mask word and nibble"
case("words", WORDS, 100, 160,
     [O(17, 48, d=16), O(17, 144, d=16), O(52, 48, d=17), O(52, 143, d=17),                         # [32, 64), [128, w), [31, 65), [126, w)
      O(72, 32), O(72, 64), O(72, 96), O(72, 128), O(72, 1), O(72, 159),                            # [32 k - 1, 32 k + 1), [0, 2), [158, 160)
      O(76, 160), O(76, -160),                                                                      # one bit: bit 31 of the last word, bit 0 of the first
      O(88, 50, d=11), O(85, 58, d=11),                                                             # a union that is no rectangle
      O(80, 85), O(80, 90), O(80, 95), O(80, 100),                                                  # starts at residues 0, 1, 2, 3 mod 4
      O(90, 120, d=11), O(90, 146, d=11)],                                                          # 22 wide from residues 1 and 3: whole nibbles inside
     rs=dict(SIZES, defaultxy=1, maxxy=40),
     named={0: (1, 33, 32, 64), 1: (1, 33, 128, 160), 2: (35, 69, 31, 65), 3: (35, 69, 126, 160), 4: (71, 73, 31, 33), 5: (71, 73, 63, 65),
            8: (71, 73, 0, 2), 9: (71, 73, 158, 160), 10: (75, 77, 159, 160), 11: (75, 77, 0, 1), 12: (77, 99, 39, 61), 13: (74, 96, 47, 69),
            14: (79, 81, 84, 86), 15: (79, 81, 89, 91), 16: (79, 81, 94, 96), 17: (79, 81, 99, 101), 18: (79, 100, 109, 131), 19: (79, 100, 135, 157)},
     seams=[("col", 32), ("col", 64), ("col", 31), ("col", 65), ("col", 128), ("col", 96), ("col", 159), ("col", 1)],
     expect=dict(delta=True, fold=True, sorted=False))
case("words_sorted", WORDS, 100, 160, CASES[-1].objs, rs=CASES[-1].rs, knobs={"LFDMI_RS_SORT_MIN": "0"}, named=CASES[-1].named,
     seams=CASES[-1].seams, expect=dict(fold=True, sorted=True, side="bands"))

# -- the 64 lanes of k_rs_fill --------------------------------------------------------------------------------------------------
FILL = "64-lane step of k_rs_fill"
case("fill_widths", FILL, 330, 416,
     [O(20, 20, d=16), O(40, 80, d=32), O(70, 200, d=60), O(10, 421), O(40, 401, d=16), O(90, 403, d=20), O(150, 385, d=32), O(225, 384, d=33),
      O(321, 30, d=16), O(321, 401, d=16), O(318, 200, d=33)], rs=dict(SIZES, maxxy=70),
     named={0: (4, 36, 4, 36), 1: (8, 72, 48, 112), 2: (10, 130, 140, 260), 3: (4, 16, 415, 416), 4: (24, 56, 385, 416), 5: (70, 110, 383, 416),
            6: (118, 182, 353, 416), 7: (192, 258, 351, 416), 8: (305, 330, 14, 46), 9: (305, 330, 385, 416), 10: (285, 330, 167, 233)},
     seams=[("col", 415), ("col", 385), ("col", 383), ("col", 353), ("col", 351), ("row", 305)], expect=dict(fold=True, sorted=False, side="two"))
case("fill_w129", FILL, 160, 320, [O(80, 256, d=65), O(150, 40, d=20)], rs=dict(SIZES, maxxy=70),
     named={0: (15, 145, 191, 320), 1: (130, 160, 20, 60)}, seams=[("col", 191), ("row", 15), ("row", 145), ("row", 130)])
FILL_WIDTHS = (1, 31, 32, 33, 63, 64, 65, 120, 129)

# -- the eight rows of a sweep workgroup and of a fill band, the sorted range ----------------------------------------------------
BANDS = "band rows and the sorted range"
case("band_phases", BANDS, 45, 256, [O(6 + k, 16 + 30 * k) for k in range(8)] + [O(39 - k, 16 + 30 * k) for k in range(8)],
     named={0: (0, 12, 10, 22), 7: (7, 19, 220, 232), 8: (33, 45, 10, 22), 15: (26, 38, 220, 232)}, seams=[("row", 4), ("row", 16), ("row", 32), ("row", 40)])
case("band_phases_sorted", BANDS, 45, 256, CASES[-1].objs, knobs={"LFDMI_RS_SORT_MIN": "0"}, named=CASES[-1].named, seams=CASES[-1].seams,
     expect=dict(sorted=True, side="bands"))
case("range_hmax", BANDS, 64, 128, [O(13, 14, d=12), O(12, 44, d=12), O(21, 78, d=12), O(20, 108, d=12)], rs=dict(SIZES, maxxy=12),
     knobs={"LFDMI_RS_SORT_MIN": "0"}, named={0: (1, 25, 2, 26), 1: (0, 24, 32, 56), 2: (9, 33, 66, 90), 3: (8, 32, 96, 120)},
     seams=[("row", 24), ("row", 25), ("row", 32), ("row", 33)], expect=dict(sorted=True, fold=True))
case("range_default_above_maxxy", BANDS, 64, 128, [O(19, 20), O(18, 60), O(40, 100, d=12), O(50, 20, d=13)], rs=dict(SIZES, defaultxy=14, maxxy=12),
     knobs={"LFDMI_RS_SORT_MIN": "0"}, named={0: (5, 33, 6, 34), 1: (4, 32, 46, 74), 2: (28, 52, 88, 112), 3: (36, 64, 6, 34)},
     seams=[("row", 32), ("row", 33), ("row", 36)], expect=dict(sorted=True, fold=True))

# -- k_rs_sort ----------------------------------------------------------------------------------------------------------------
SORT = "k_rs_sort"


def sort_objs(h):
    """Squares of 12 rows in four columns of a 64-wide frame; first rows at the ends of the frame and around the rows where a
    thread's share of the scan and a wave's begin (multiples of ``per``, of 64 ``per``, 1023 / 1024)."""
    a = [0, 13, 26, 511, 524, 2035, 2048, h - 12]
    b = [1, 500, 2047, 2061, h - 1]
    objs = []
    for firsts, y in ((a, 8), (b, 24), ([1023, 1040], 40), ([1024, 1037], 56)):
        last = -100
        for f in sorted(set(firsts)):
            if 0 <= f < h and f >= last + 12:
                objs.append(O(f + 6, y))
                last = f
    return objs


case("sort_h7", SORT, 7, 32, [O(6, 16), O(9, 26)], knobs={"LFDMI_RS_SORT_MIN": "0"}, named={0: (0, 7, 10, 22), 1: (3, 7, 20, 32)}, batch=False,
     seams=[("row", 3), ("col", 10)])
for _h in (1023, 1024, 1025, 2100):
    case(f"sort_h{_h}", SORT, _h, 64, sort_objs(_h), knobs={"LFDMI_RS_SORT_MIN": "0"}, named={0: (0, 12, 2, 14)},
         seams=[("row", 12), ("row", _h - 1), ("row", _h - 12)], expect=dict(sorted=True, fold=True, side="bands"))
case("sort_one_first_row", SORT, 64, 256, [O(20, 6 + 6 * i) for i in range(40)], knobs={"LFDMI_RS_SORT_MIN": "0"},
     named={0: (14, 26, 0, 12), 39: (14, 26, 234, 246)}, seams=[("row", 14), ("row", 26), ("col", 246)], expect=dict(sorted=True))
case("sort_all_stay", SORT, 40, 160, [O(10 + i % 20, 10 + 7 * i, nobs=2) for i in range(20)], knobs={"LFDMI_RS_SORT_MIN": "0"},
     named={i: None for i in range(20)}, nothing=True, expect=dict(sorted=True))
CROWD_SIZES = (1, 3, 4, 5, 255, 256, 257)


def crowd_objs(n, h=100, w=256, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    xs, ys = rng.uniform(-20, h + 20, n), rng.uniform(-20, w + 20, n)
    if n <= 5:                                   # the few objects of a small catalogue all leave a square
        xs, ys = rng.uniform(6, h - 6, n), rng.uniform(6, w - 6, n)
    return [O(float(xs[i]), float(ys[i]), nobs=1 + (i % 3 == 2 and n > 5)) for i in range(n)]


for _n in CROWD_SIZES:
    case(f"crowd_{_n}", "catalogue size (blocks of 4 and 256 objects)", 100, 256, crowd_objs(_n), expect=dict(sorted=False, side="two"))
    case(f"crowd_{_n}_sorted", "catalogue size (blocks of 4 and 256 objects)", 100, 256, crowd_objs(_n), knobs={"LFDMI_RS_SORT_MIN": "0"},
         expect=dict(sorted=True, side="bands"))

# -- routes by shape ----------------------------------------------------------------------------------------------------------
SHAPE = "routes by shape"
case("w4128", SHAPE, 24, 4128, [O(6, 10), O(14, 2050), O(6, 4096), O(14, 4122), O(6, 4133)], knobs={"LFDMI_RS_SORT_MIN": "0"},
     named={2: (0, 12, 4090, 4102), 4: (0, 12, 4127, 4128)}, seams=[("col", 4090), ("col", 4127), ("row", 12)],
     expect=dict(delta=True, fold=False, sorted=False, side=None))                  # w > RS_MAXW: the fill in front, per object
for _w in (100, 136):
    case(f"w{_w}", SHAPE, 40, _w, [O(10, 20), O(25, _w - 6), O(20, _w + 5), O(-8, 60)], knobs={"LFDMI_RS_SORT_MIN": "0"},
         named={1: (19, 31, _w - 12, _w), 2: (14, 26, _w - 1, _w), 3: (26, 38, 54, 66)}, seams=[("col", _w - 1), ("col", _w - 12)],
         expect=dict(delta=False, fold=False, sorted=False, side=None))             # w % 32: no bit planes, no sort
case("w4096", SHAPE, 16, 4096, [O(6, 10), O(10, 2048), O(6, 4090), O(10, 4101), O(-8, 3000)], named={2: (0, 12, 4084, 4096), 3: (4, 16, 4095, 4096), 4: (2, 14, 2994, 3006)},
     seams=[("col", 4095), ("col", 4084)], expect=dict(delta=True, fold=True, sorted=False, side="two"))
case("w4096_sorted", SHAPE, 16, 4096, CASES[-1].objs, knobs={"LFDMI_RS_SORT_MIN": "0"}, named=CASES[-1].named, seams=CASES[-1].seams,
     expect=dict(delta=True, fold=True, sorted=True, side="bands"))

# -- the catalogue tests of k_rs_boxes ----------------------------------------------------------------------------------------
CAT = "catalogue tests of k_rs_boxes"
CAT_BLOTTED = {0: (2, 14), 3: (2, 14), 4: (2, 14), 6: (0, 40), 7: (24, 36), 9: (24, 36)}   # object -> its rows; the others stay


def cat_objs(filter):
    """Ten objects, one per branch; the centres differ from filter to filter (column f holds base + f), the others' columns
    hold a centre far outside the frame."""
    f = FILTERS.index(filter)
    cap = CAPS[filter]
    top = float(math.ceil(cap))                  # the smallest ceil'ed magnitude that is not below the cap (the cap itself for 'u')
    def pos(x, y):                                                                         # noqa: E306
        xs, ys = np.full(5, 900.0), np.full(5, 900.0)
        xs[f], ys[f] = x, y + f
        return xs, ys
    def mags(own, others=15.0):                                                           # noqa: E306
        m = np.full(5, others)
        m[f] = own
        return m
    pairs3, pairs4 = np.array([15.0, 15, 15, 19, 17]), np.array([15.0, 15, 15, 15, 19])
    return [O(*pos(8, 10)),                                                                # 0 blotted
            O(*pos(8, 24), mags=np.full(5, top)),                                          # 1 at the cap (equal for 'u'): stays
            O(*pos(8, 38), mags=np.full(5, np.nextafter(np.float32(top), np.float32(0)))),  # 2 just under it as float32, equal after ceil: stays
            O(*pos(8, 52), mags=np.full(5, top - 1)),                                      # 3 one below: blotted
            O(*pos(8, 66), mags=np.roll(pairs3, f - 3)),                                   # 4 three differences above maxmagdiff == magcount: blotted
            O(*pos(8, 80), mags=np.roll(pairs4, f - 4)),                                   # 5 four: stays
            O(*pos(25, 130), pet=5.2),                                                     # 6 ceil 6 -> int(6 / 0.396) + 10 == 25 == maxxy
            O(*pos(30, 20), pet=6.5),                                                      # 7 ceil 7 -> 27 > maxxy: the default
            O(*pos(30, 40), nobs=2),                                                       # 8 NOBSERVE != NDETECT: stays
            O(*pos(29.3, 59.2))]                                                           # 9 fractional centres: ceil


for _f in FILTERS:
    _k = FILTERS.index(_f)
    case(f"cat_{_f}", CAT, 40, 160, cat_objs(_f), filter=_f,
         named={0: (2, 14, 4 + _k, 16 + _k), 1: None, 2: None, 3: (2, 14, 46 + _k, 58 + _k), 4: (2, 14, 60 + _k, 72 + _k), 5: None,
                6: (0, 40, 105 + _k, 155 + _k), 7: (24, 36, 14 + _k, 26 + _k), 8: None, 9: (24, 36, 54 + _k, 66 + _k)},
         seams=[("row", 14), ("row", 24), ("col", 105 + _k)])

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ---- batches ----------------------------------------------------------------------------------------------------------------
# five 40 x 160 frames with five different catalogues through a two-slot context (cat_f0 + c0): counts of 5, 0, 1, 8 and 5 under a
# max_obj of 8, so a frame without objects and one with a single object ("ONE": BATCH_SMALLER) sit beside crowded neighbours, and
# the last chunk's frame, whose stage images are fetched, has squares
BATCH5 = ("wrap_rows", None, "ONE", "slice_exact", "wrap_cols")
BATCH_BIGGER = [O(float(x), float(y), nobs=1 + (i % 4 == 3)) for i, (x, y) in
                enumerate(zip(np.random.default_rng(77).uniform(-20, 60, 40), np.random.default_rng(78).uniform(-20, 180, 40)))]
BATCH_SMALLER = [O(20, 80)]
# the children: LFDMI_PREP_ROWS and LFDMI_RS_FILL_FRAC are read once per process
CHILD_CASES = ("wrap_rows", "words", "band_phases", "crowd_5")
CHILD_ENVS = ({"LFDMI_PREP_ROWS": "1"}, {"LFDMI_PREP_ROWS": "4"}, {"LFDMI_PREP_ROWS": "16"}, {"LFDMI_RS_FILL_FRAC": "0"},
              {"LFDMI_RS_FILL_FRAC": "0.3"}, {"LFDMI_RS_FILL_FRAC": "1"})
# frames that overflow a context with tiny tables and are run again alone (big-endian: with their catalogue row)
SPILL_CASES = ("crowd_255", "crowd_5", "crowd_257")
SPILL_CAPS = {"run_cap": 500, "key_cap": 50, "slot_cap": 500, "list_cap": 300, "peak_cap": 64}


BATCH8_SHAPE = (80, 448)                        # (a Hough line needs more room than the 40 x 160 of the slice cases)


def streak(h=80, w=448):
    """A frame the bright pass decides: a bright line on sky that prep clips to zero (slightly negative, so the squares still
    show in the frame the caller gets back)."""
    f = fc.blank(h, w, 70)
    yy, xx = np.mgrid[0:h, 0:w]
    f[np.abs(yy - (0.12 * xx + 8)) < 2.0] = fc.AMPS[3]
    return f


BATCH8 = ("wrap_rows", "STREAK", "wrap_cols", "slice_exact", "STREAK", "slice_empty", "ONE", "slice_exact")
BATCH8_STREAK_CAT = [O(70, 40), O(-8, 300), O(72, 446)]                           # (squares that leave the line alone)


def batch_cat(name):
    """The catalogue of one batch entry: a named case's, the single object of BATCH_SMALLER ("ONE") or none at all (None)."""
    return None if name is None else catalogue(BATCH_SMALLER) if name == "ONE" else BY_NAME[name].cat


def batch8():
    """[(frame, catalogue)] of the eight slots: the catalogues of the named cases on 80 x 448 flat frames, and the streak."""
    return [(streak(), catalogue(BATCH8_STREAK_CAT)) if n == "STREAK" else (flat(*BATCH8_SHAPE), batch_cat(n)) for n in BATCH8]


NOT_REACHED = {
    "h >= RS_SORT_MAXH": "8192 rows: check_shape refuses heights above 8191, so the sort's h < RS_SORT_MAXH is always true",
    "prep_rows > RS_MAXROWS": "LFDMI_PREP_ROWS takes 1, 2, 4, 8 or 16 only",
    "a whole pass on the 7-row frame": "sort_h7 is named for k_rs_sort, which lfdmi_remove_stars reaches, and goes through that entry point only; the "
                                       "lowest frames that run whole passes are w4096 (16 rows) and short_h_lt_d (17 rows)",
    "non-finite catalogue values": "refused by the host layer (_check_finite) before they reach the library",
    "the last row or column by the wrap": "a wrapped slice stops at -1 at the latest: it ends one short of the far edge (wrap_rows, wrap_cols)",
}
