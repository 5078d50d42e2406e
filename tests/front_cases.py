"""Named front-end cases, their stage-by-stage reference and a plain restatement of which kernels the host launches for them.

The front end of a pass is prep -> equalise -> (dim: erode) -> dilate -> Canny -> contours / rectangles.  ``reference`` builds
every stage image from the oracle's operators, one after the other; ``route`` restates the host's choice of kernels
(lfdmi.hip: can_fuse_dilate_canny, run_dilate_canny, prep_erode_rows, can_fuse_prep_erode, dim_front_end, run_front, run_morph)
for a shape, a parameter set, the LFDMI_* knobs and the stage-image mode; ``active_tiles`` restates k_dc_tiles.  Nothing here
touches the device: tests/test_front_cases_model.py checks on the CPU that every case of ``CASES`` takes the route and crosses
the constant it is named for and is not vacuous, tests/test_gpu_front_seams.py runs them on the device against the reference.

Frames are small and crafted: exact zeros (slightly negative noise, which every prep mode clips) with bars, blobs, single
pixels and hollow squares of a few distinct amplitudes, so that the equalised levels are far apart and the features sit on
both sides of the seam a case names.  ``frame`` is what the kernels see after the vertical flip; the entry points get
``frame[::-1]`` with flip on, the way the batch path always runs.
"""
import numpy as np

# ---- constants of the kernels (k_image.h, k_dcw_tile.inc, k_ccl.h, k_frame.h, include/lfdmi.h) ---------------------------
CANNY_TW, DCW_TH, CANNY_HALO, DCW_MAXKH, DCT_MAXBANDS = 64, 16, 16, 13, 512
CELL, CELLBM_WORDS = 16, 8                      # 16 x 16 cells, 512 of them per band (8 words of 64)
MORPH_TW, MORPH_TH = 64, 32                     # tiles of k_erode_cand / k_morph_rect_rows / k_fill_around
MAX_MORPH_K = 31
PE_ROWS = 12                                    # rows per band of k_prep_erode before prep_erode_rows shortens them
SCAN_WORDS_PER_WG = 4 * 8 * 64                  # SCANW_WAVES x SCAN_SEGS segments of 64 words per workgroup of k_scan_fused
FRAME_RUNCAP, FRAME_HOLECAP = 32768, 1024
MAX_SIDE = 8191                                 # check_shape: no context takes a wider or taller frame
C_NQUADS, C_NRUNF, C_NRUNB, C_NTILES = 2, 12, 13, 17                      # LFDMI_COUNTERS slots the tests read
MAX_PIXELS = 700_000

ONES = lambda kh, kw: np.ones((kh, kw), np.uint8)   # noqa: E731
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)


def default_params():
    from lfd_amd.detecttrails import default_params as dp
    pb, pd, _ = dp()
    return pb, pd


# ---- the host's choice of kernels ----------------------------------------------------------------------------------------

def all_ones(k):
    return bool(np.all(np.asarray(k) != 0))


def can_fuse_dilate_canny(kernel, w):
    kh, kw = kernel.shape
    if kh > MAX_MORPH_K or kw > MAX_MORPH_K or w % 16 or not all_ones(kernel):
        return False
    ax = kw // 2
    return ax + 4 <= CANNY_HALO and (kw - 1 - ax) + 4 <= CANNY_HALO


def prep_erode_rows(w, kh, pe_rows=PE_ROWS):
    br = pe_rows
    while br > 2 and (2 * br + kh - 1) * (w + 32) > 60 * 1024:
        br >>= 1
    if (2 * br + kh - 1) * (w + 32) + 16 > 140 * 1024:
        return 0
    return br if br >= 2 * (kh - 1) else 0


def can_fuse_prep_erode(w, kernel, keep, knobs):
    if not int(knobs.get("LFDMI_FUSE_PREP_ERODE", 1)) or keep or w % 16:
        return False
    kh, kw = kernel.shape
    if kh > MAX_MORPH_K or kw > MAX_MORPH_K or not all_ones(kernel):
        return False
    return kw // 2 <= 16 and kw - 1 - kw // 2 <= 16 and prep_erode_rows(w, kh) > 0


def route(h, w, params, entry, mode, knobs=None):
    """What run_front launches for one h x w float32 frame.  entry: "bright" / "dim" (lfdmi_process_*) or "batch" (the dim pass of
    lfdmi_detect_batch); mode: lfdmi_set_stage_images (0: no 8-bit stage images, 1: all).  Returns a dict:
    front  "prep" (k_prep_hist alone, bright), "band" (k_prep_erode), "bits" (bright sweep's bit planes + k_bits_erode),
           "erode" (k_prep_hist + k_morph_rect_v / k_morph_rect / k_morph_generic), "wide" (k_prep_hist + k_erode_cand +
           k_morph_rect_rows, and k_fill_around when only_tiles)
    band_rows  rows per band of k_prep_erode (front == "band"), else 0
    only_tiles the eroded plane is zero-filled only around the marked cells (so ERODED cannot be fetched)
    dc     "tiles" (k_dc_tiles + k_dilate_canny_t), "strips" (k_dilate_canny_w), "v" (k_dilate_canny_v), "separate" (a dilation
           kernel + k_canny_nms)
    spec   the tile kernel's instantiation: (4, 4), (9, 9) or (0, 0)
    parts  waves per frame of k_dilate_canny_t
    fetch  the stage images lfdmi_get_stage hands out afterwards."""
    knobs = knobs or {}
    flag = lambda k, d=1: bool(int(knobs.get(k, d)))                                # noqa: E731
    keep = mode == 1
    dim = entry != "bright"
    dk = params["dilateKernel"]
    tiles_x, tiles_y = -(-w // CANNY_TW), -(-h // DCW_TH)
    tilelist = flag("LFDMI_DC_TILELIST") and tiles_x <= 128 and tiles_y <= DCT_MAXBANDS
    fused_dc = can_fuse_dilate_canny(dk, w)
    r = dict(front="prep", band_rows=0, only_tiles=False)
    if dim:
        ek = params["erodeKernel"]
        ekh, ekw = ek.shape
        fuse_pe = can_fuse_prep_erode(w, ek, keep, knobs)
        delta = (entry == "batch" and not flag("LFDMI_FUSE_DUAL", 0) and flag("LFDMI_DELTA_DIM") and w % 32 == 0
                 and 0.0 <= np.float32(params["addFlux"]) <= np.float32(0.999) and np.float32(params["minFlux"]) <= np.float32(0.5)
                 and ekh * ekw <= 25 and fuse_pe)
        if delta:
            r["front"] = "bits"
        elif fuse_pe:
            r["front"], r["band_rows"] = "band", prep_erode_rows(w, ekh)
        else:
            wide = ekw >= 7 and w % 4 == 0 and ekh <= 33 and all_ones(ek) and w % 16 == 0 and -(-w // MORPH_TW) <= 128
            r["front"] = "wide" if wide else "erode"
            r["only_tiles"] = bool(wide and not keep and flag("LFDMI_SPARSE_ERODE_FILL") and flag("LFDMI_CELLBM") and tilelist
                                   and dk.shape[0] <= 9 and fused_dc and ekh <= 9)
    if not fused_dc:
        r["dc"] = "separate"
    elif dk.shape[0] > DCW_MAXKH:
        r["dc"] = "v"
    else:
        r["dc"] = "tiles" if tilelist else "strips"
    spec = flag("LFDMI_DC_SPECIALIZE") and dk.shape in ((4, 4), (9, 9))
    r["spec"] = dk.shape if (r["dc"] == "tiles" and spec) else (0, 0)
    r["parts"] = int(knobs.get("LFDMI_DC_PARTS", 0)) or max(8, min(256, tiles_x * tiles_y // 8))
    fetch = ["CANNY", "BOX"]
    if keep:
        fetch += ["GRAY", "EQUALIZED", "EQU"] + (["ERODED"] if dim else [])
    elif dim and not r["only_tiles"]:
        fetch.append("ERODED")
    r["fetch"] = fetch
    return r


def active_tiles(src):
    """k_dc_tiles on the cell marks of ``src`` (the image the fused dilate + Canny kernel reads: the 8-bit image of the bright
    pass, the eroded one of the dim pass): tile (ty, tx) is listed when a marked 16 x 16 cell lies in cells 4 tx - 1 .. 4 tx + 4
    of bands ty - 1 .. ty + 1.  Returns the boolean tile map [tiles_y, tiles_x]."""
    h, w = src.shape
    by, bx = -(-h // CELL), -(-w // CELL)
    pad = np.zeros((by * CELL, bx * CELL), bool)
    pad[:h, :w] = src != 0
    cells = pad.reshape(by, CELL, bx, CELL).any(axis=(1, 3))
    tiles_x, tiles_y = -(-w // CANNY_TW), -(-h // DCW_TH)
    out = np.zeros((tiles_y, tiles_x), bool)
    for ty in range(tiles_y):
        rows = cells[max(0, ty - 1):ty + 2].any(axis=0)
        for tx in range(tiles_x):
            out[ty, tx] = rows[max(0, 4 * tx - 1):4 * tx + 5].any()
    return out


# ---- the reference ---------------------------------------------------------------------------------------------------------

def reference(O, frame, params, dim):
    """Every stage image of one pass on ``frame`` (already flipped), from the oracle's operators one after the other."""
    mode = O.PREP_BRIGHT_THEN_DIM if dim else O.PREP_BRIGHT
    gray = O.prep(frame, mode, False, params.get("minFlux", 0.0) if dim else 0.0, params.get("addFlux", 0.0) if dim else 0.0)
    equalized = O.equalize_hist(gray)
    eroded = O.erode(equalized, params["erodeKernel"]) if dim else None
    equ = O.dilate(eroded if dim else equalized, params["dilateKernel"])
    edges = O.canny(equ, 0, 255)
    det, box, nb = O.fit_min_area_rect(equ, params["contoursMode"], params["contoursMethod"], params["minAreaRectMinLen"], params["lwTresh"])
    return dict(GRAY=gray, EQUALIZED=equalized, ERODED=eroded, EQU=equ, CANNY=edges, BOX=box, detection=det, n_boxes=nb)


# ---- frames ----------------------------------------------------------------------------------------------------------------

AMPS = (60.0, 110.0, 160.0, 215.0)             # far apart after equalisation: steps between any two exceed Canny's upper threshold / 4


def blank(h, w, seed=0):
    """Low noise that every prep mode clips to an exact zero."""
    rng = np.random.default_rng(seed)
    return (-np.abs(rng.normal(0.0, 0.05, (h, w))) - 0.01).astype(np.float32)


def box(f, y0, y1, x0, x1, amp):
    """Rows y0 .. y1, columns x0 .. x1 inclusive, clipped to the frame."""
    h, w = f.shape
    f[max(0, y0):min(h, y1 + 1), max(0, x0):min(w, x1 + 1)] = amp


def hollow(f, y0, y1, x0, x1, t, amp):
    box(f, y0, y0 + t - 1, x0, x1, amp)
    box(f, y1 - t + 1, y1, x0, x1, amp)
    box(f, y0, y1, x0, x0 + t - 1, amp)
    box(f, y0, y1, x1 - t + 1, x1, amp)


class Case:
    """One frame, one parameter set, one set of knobs.  seam: ("row" | "col", index): features lie on both sides of the line
    between index - 1 and index.  entries: which of "bright", "dim", "batch" the device test runs.  expect: what the model test
    asserts about the route, e.g. dict(entry="dim", mode=0, front="band", band_rows=12)."""

    def __init__(self, name, row, build, entries=("bright", "dim", "batch"), dilate=None, erode=None, knobs=None, seams=(), expect=(),
                 survivors=(), vanish=(), box_expected=None, ntiles=None, holes=None, flux=None):
        self.name, self.row, self.build, self.entries = name, row, build, tuple(entries)
        self.dilate, self.erode, self.knobs = dilate, erode, dict(knobs or {})
        self.seams, self.expect = tuple(seams), tuple(expect)
        self.survivors, self.vanish, self.box_expected = tuple(survivors), tuple(vanish), box_expected
        self.ntiles, self.holes, self.flux = ntiles, holes, flux
        self._frame = None

    def __repr__(self):
        return self.name

    @property
    def frame(self):
        if self._frame is None:
            f = self.build()
            assert f.dtype == np.float32 and f.size <= MAX_PIXELS
            f.setflags(write=False)
            self._frame = f
        return self._frame

    def params(self, entry):
        """The parameter dict of one entry.  "batch" gives (bright that never fits a rectangle, dim): every frame reaches the
        dim pass."""
        pb, pd = default_params()
        if self.dilate is not None:
            pb["dilateKernel"] = self.dilate
            pd["dilateKernel"] = self.dilate
        if self.erode is not None:
            pd["erodeKernel"] = self.erode
        if self.flux is not None:
            pd["minFlux"], pd["addFlux"] = self.flux
        if entry == "bright":
            return pb
        if entry == "dim":
            return pd
        return dict(pb, lwTresh=1e9), pd


CASES = []


def case(*a, **k):
    CASES.append(Case(*a, **k))


# -- the 64 x 16 tile of the fused dilate + Canny kernel ----------------------------------------------------------------------

def f_tile_pixels():
    f = blank(48, 192, 1)
    f[15, 63], f[16, 64] = AMPS[3], AMPS[2]
    box(f, 31, 32, 127, 128, AMPS[1])                       # 2 x 2 over four tiles
    return f


def f_staircase(h=64, w=256, seed=2):
    """Bars whose boundaries take every phase against rows 16 k and columns 64 k."""
    f = blank(h, w, seed)
    for k in range(8):
        box(f, 9 + k, 15 + k, 4 + 14 * k, 13 + 14 * k, AMPS[k % 4])       # lower edges on rows 15 .. 22
        box(f, 27 + k, 33 + k, 4 + 14 * k, 13 + 14 * k, AMPS[(k + 1) % 4])  # upper edges on rows 27 .. 34 (32 = 2 x 16)
    for k in range(8):
        box(f, 40 + 3 * (k % 2), 50 + 3 * (k % 2), 121 + k * 13, 127 + k * 13, AMPS[(k + 2) % 4])
    box(f, 52, 62, 188, 196, AMPS[0])                       # across column 192 = 3 x 64
    box(f, 14, 20, 120, 136, AMPS[1])                       # across column 128: its upper and lower edges cross it at any dilation
    box(f, 58, 60, 8, 112, AMPS[3])                         # long and thin: a rectangle for the BOX image
    return f


def f_halo8():
    """3 x 3 tiles; eight 5 x 5 blobs just inside the centre tile (rows 16 .. 31, columns 64 .. 127), one per direction: the
    neighbour sees each only through its halo."""
    f = blank(48, 192, 3)
    ys, xs = (16, 22, 27), (64, 94, 123)
    n = 0
    for i, y in enumerate(ys):
        for j, x in enumerate(xs):
            if i == 1 and j == 1:
                continue
            box(f, y, y + 4, x, x + 4, AMPS[n % 4])
            n += 1
    return f


def f_borders(h, w, seed):
    f = blank(h, w, seed)
    box(f, 0, 3, 6, w // 2, AMPS[0])                       # row 0
    box(f, h - 4, h - 1, w // 3, w - 7, AMPS[1])           # row h - 1
    box(f, 6, h - 7, 0, 3, AMPS[2])                        # column 0
    box(f, 8, h - 9, w - 4, w - 1, AMPS[3])                # column w - 1
    box(f, h // 2 - 2, h // 2 + 2, w // 2 - 3, w // 2 + 3, AMPS[3])
    return f


TILE = "tile of the fused dilate + Canny"
case("tile_pixels", TILE, f_tile_pixels, entries=("bright",), seams=[("row", 16), ("col", 64), ("row", 32), ("col", 128)],
     expect=[dict(entry="bright", mode=0, dc="tiles", spec=(4, 4))])
case("tile_staircase", TILE, f_staircase, seams=[("row", 16), ("row", 32), ("col", 128), ("col", 192)], box_expected=True,
     expect=[dict(entry="bright", mode=0, dc="tiles", spec=(4, 4)), dict(entry="dim", mode=0, dc="tiles", spec=(9, 9), front="band"),
             dict(entry="batch", mode=0, front="bits"), dict(entry="dim", mode=1, front="erode")])
case("tile_halo8", TILE, f_halo8, seams=[("row", 16), ("row", 32), ("col", 64), ("col", 128)])
for _h, _w in ((33, 80), (47, 96), (17, 112), (31, 208)):
    case(f"tile_borders_{_h}x{_w}", TILE, (lambda h=_h, w=_w: f_borders(h, w, h + w)),
         seams=[("row", 16)] + ([("col", 64)] if _w > 64 else []), survivors=[(0, 10), (_h - 1, _w // 3 + 4)] if _h > 17 else [])
for _n in ("tile_staircase", "tile_halo8", "tile_borders_47x96"):
    _c = next(c for c in CASES if c.name == _n)
    case(_n + "_strips", "more than 128 tile columns (k_dilate_canny_w by knob)", _c.build, knobs={"LFDMI_DC_TILELIST": "0"}, seams=_c.seams,
         expect=[dict(entry="bright", mode=0, dc="strips"), dict(entry="dim", mode=0, dc="strips")])

# -- the reach of the tile list -----------------------------------------------------------------------------------------------

REACH = "tile list reach"
REACH_SPOTS = dict(left=(38, 188), right=(38, 256), top=(28, 220), bottom=(48, 220), top_left=(28, 188), top_right=(28, 256),
                   bottom_left=(48, 188), bottom_right=(48, 256))


def f_reach(side):
    """5 bands x 7 tiles; the target tile is (2, 3): rows 32 .. 47, columns 192 .. 255, reached from cells 11 .. 16 of bands
    1 .. 3.  One 4 x 4 blob in the outermost cell of that reach, hard against the tile, and nothing else."""
    f = blank(80, 448, 5)
    y, x = REACH_SPOTS[side]
    box(f, y, y + 3, x, x + 3, AMPS[3])
    return f


for _s in REACH_SPOTS:
    case(f"reach_{_s}", REACH, (lambda s=_s: f_reach(s)),
         seams=[("col", 192)] if _s == "left" else [("col", 256)] if _s == "right" else [("row", 32)] if _s == "top" else [("row", 48)] if _s == "bottom" else [],
         expect=[dict(entry="bright", mode=0, dc="tiles", parts=8)])
case("reach_none", REACH, lambda: blank(80, 448, 6), ntiles=0)


def f_all_tiles():
    f = blank(48, 192, 7)
    for y in range(13, 48, 16):
        for x in range(13, 192, 16):
            box(f, y, y + 3, x, x + 3, AMPS[(x // 16 + y // 16) % 4])
    return f


case("reach_all", REACH, f_all_tiles, ntiles=9, seams=[("row", 16), ("col", 64)])

# -- the word of the cell bitmap, the second ballot half ----------------------------------------------------------------------

def f_cellword(which):
    f = blank(32, 1088, 8)
    if which in ("left", "across"):
        box(f, 8, 12, 1019, 1023, AMPS[3])                   # cell 63 only: tile 16 sees it through bits 63 .. of word 0
    if which in ("right", "across"):
        box(f, 20, 24, 1024, 1028, AMPS[2])                  # cell 64 only: tile 15 reaches it in word 1
    if which == "across":
        box(f, 14, 18, 1004, 1044, AMPS[1])
    return f


for _s in ("left", "right", "across"):
    case(f"cellword_{_s}", "cell-bitmap word", (lambda s=_s: f_cellword(s)), seams=[("col", 1024)],
         expect=[dict(entry="bright", mode=0, dc="tiles")])
case("cellword_across_strips", "cell-bitmap word", lambda: f_cellword("across"), seams=[("col", 1024)], knobs={"LFDMI_DC_TILELIST": "0"},
     expect=[dict(entry="bright", mode=0, dc="strips")])


def f_ballot():
    f = blank(32, 4160, 9)
    box(f, 6, 11, 4090, 4110, AMPS[3])
    box(f, 18, 22, 4092, 4095, AMPS[1])
    box(f, 20, 26, 4140, 4159, AMPS[2])                      # the last tile, up to the last column
    box(f, 12, 16, 2040, 2052, AMPS[0])
    return f


case("ballot_half", "second ballot half", f_ballot, seams=[("col", 4096)], expect=[dict(entry="bright", mode=0, dc="tiles")])

# -- a wave's share of the tile list ------------------------------------------------------------------------------------------

def f_share(n):
    """80 x 4160: 5 bands of 65 tiles.  A blob in the middle of a tile of band 0 lists that tile and the one below it; a blob in
    band 2 lists three (bands 1 .. 3): n = 2 a (+ 3)."""
    f = blank(80, 4160, 10 + n)
    a, odd = (n - 3) // 2 if n % 2 else n // 2, n % 2
    for tx in range(a):
        box(f, 6, 9, 64 * tx + 22, 64 * tx + 25, AMPS[tx % 4])
    if odd:
        box(f, 38, 41, 64 * 64 + 22, 64 * 64 + 25, AMPS[3])
    return f


for _n in (64, 65, 128, 129):
    case(f"share_{_n}", "a wave's share of the list", (lambda n=_n: f_share(n)), entries=("bright", "dim"), knobs={"LFDMI_DC_PARTS": "1"}, ntiles=_n,
         expect=[dict(entry="bright", mode=0, dc="tiles", parts=1)])

# -- the size of the dilation -------------------------------------------------------------------------------------------------

DIL = "dilate kernel size"
for _kh, _kw, _dc, _spec in ((4, 4, "tiles", (4, 4)), (9, 9, "tiles", (9, 9)), (1, 1, "tiles", (0, 0)), (3, 3, "tiles", (0, 0)), (2, 7, "tiles", (0, 0)),
                             (5, 5, "tiles", (0, 0)), (13, 13, "tiles", (0, 0)), (13, 25, "tiles", (0, 0)), (14, 3, "v", (0, 0)), (3, 27, "separate", (0, 0))):
    case(f"dilate_{_kh}x{_kw}", DIL, f_staircase, entries=("bright", "dim"), dilate=ONES(_kh, _kw), seams=[("row", 16), ("row", 32), ("col", 128)],
         expect=[dict(entry="bright", mode=0, dc=_dc, spec=_spec), dict(entry="dim", mode=1, dc=_dc, spec=_spec)])
for _k in (4, 9):
    case(f"dilate_{_k}x{_k}_runtime", DIL, f_staircase, entries=("bright", "dim"), dilate=ONES(_k, _k), knobs={"LFDMI_DC_SPECIALIZE": "0"},
         seams=[("row", 16), ("col", 128)], expect=[dict(entry="bright", mode=0, dc="tiles", spec=(0, 0))])
case("dilate_cross", DIL, f_staircase, entries=("bright", "dim"), dilate=CROSS, seams=[("row", 16)], expect=[dict(entry="bright", mode=0, dc="separate")])
case("dilate_w250", DIL, lambda: f_staircase(64, 250, 4), seams=[("row", 16), ("col", 128)],
     expect=[dict(entry="bright", mode=0, dc="separate"), dict(entry="dim", mode=0, dc="separate", front="erode")])

# -- the band of k_prep_erode -------------------------------------------------------------------------------------------------

def f_bands(h=37, w=512, rows=(12, 24), seed=20):
    """Blocks that survive a 5 x 5 erosion, their edges at every phase against the band rows; survivors on row 0 and row h - 1."""
    f = blank(h, w, seed)
    for r in rows:
        for k in range(7):
            box(f, r - 7 + k, r - 1 + k, 8 + 24 * k + 200 * (rows.index(r) % 2), 19 + 24 * k + 200 * (rows.index(r) % 2), AMPS[k % 4])
    box(f, 0, 5, 420, 431, AMPS[2])
    box(f, h - 6, h - 1, 440, 452, AMPS[3])
    box(f, h - 6, h - 1, 0, 8, AMPS[1])                     # ... and in the corner
    box(f, 28, 33, 20, 190, AMPS[0])                        # long and thin after any of the erosions: a rectangle for the BOX image
    return f


BAND = "band of k_prep_erode"
for _kh, _kw in ((3, 3), (5, 5), (3, 5), (5, 3), (2, 2)):
    case(f"band_{_kh}x{_kw}", BAND, f_bands, entries=("dim",), erode=ONES(_kh, _kw), seams=[("row", 12), ("row", 24), ("row", 36)],
         survivors=[(0, 425), (36, 446), (36, 3)], box_expected=True,
         expect=[dict(entry="dim", mode=0, front="band", band_rows=12), dict(entry="dim", mode=1, front="erode")])
case("band_w4096", BAND, lambda: f_bands(40, 4096, (6, 12), 21), entries=("dim",), seams=[("row", 6), ("row", 12)], survivors=[(0, 425), (39, 446)],
     expect=[dict(entry="dim", mode=0, front="band", band_rows=6)])

# -- the word of k_bits_erode -------------------------------------------------------------------------------------------------

def f_bits():
    """40 x 160 (the last 64-pixel word is half empty).  Blocks over columns 62 .. 66 and in the last word; inside them the
    fractional parts .2 and .6 alternate: with addFlux 0.5 the dim value is the bright value + 1 on the first and equal on the
    second.  Thin runs (1 .. 4 wide) next to the word boundary vanish or survive depending on the erosion."""
    f = blank(40, 160, 30)
    yy, xx = np.mgrid[0:40, 0:160]
    frac = np.where((yy + xx) % 2 == 0, np.float32(0.2), np.float32(0.6))
    def fbox(y0, y1, x0, x1, amp):                                                        # noqa: E306
        f[y0:y1 + 1, x0:x1 + 1] = amp + frac[y0:y1 + 1, x0:x1 + 1]
    fbox(2, 9, 56, 72, 60.0)                                 # over the first word boundary
    fbox(12, 19, 62, 66, 110.0)                              # exactly columns 62 .. 66
    fbox(22, 29, 120, 136, 160.0)                            # over the second
    fbox(30, 39, 146, 159, 215.0)                            # the half-empty last word, bottom right corner
    fbox(0, 6, 0, 9, 110.0)                                  # top left corner
    for k in range(4):
        fbox(12, 19, 100 + 7 * k, 100 + 7 * k + k, 160.0)    # runs 1 .. 4 wide
        fbox(33 + k // 2, 33 + k // 2 + k, 60 + 9 * (k % 2), 68 + 9 * (k % 2), 60.0)  # 1 .. 4 tall, across column 64
    return f


BITS = "word of k_bits_erode"
for _kh, _kw in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (3, 7)):
    case(f"bits_{_kh}x{_kw}", BITS, f_bits, entries=("batch",), erode=ONES(_kh, _kw), seams=[("col", 64), ("col", 128)], survivors=[(5, 64), (36, 155)],
         expect=[dict(entry="batch", mode=0, front="bits"), dict(entry="batch", mode=1, front="wide" if _kw >= 7 else "erode")])
    case(f"bits_{_kh}x{_kw}_second_sweep", BITS, f_bits, entries=("batch",), erode=ONES(_kh, _kw), knobs={"LFDMI_DELTA_DIM": "0"}, seams=[("col", 64)],
         expect=[dict(entry="batch", mode=0, front="band")])
case("bits_addflux_0.3", BITS, f_bits, entries=("batch",), flux=(0.02, 0.3), seams=[("col", 64)], expect=[dict(entry="batch", mode=0, front="bits")])

# -- the wide erosion ---------------------------------------------------------------------------------------------------------

def f_wide(h, w, k, seed):
    """Blobs of k .. k + 3 pixels a side on the corners of the 64 x 32 erosion tiles and in the frame's corners; one of k - 1,
    which must vanish."""
    f = blank(h, w, seed)
    n = 0
    for y in range(32, h, 32):
        for x in range(64, min(w, 64 * 5), 64):
            s = k + n % 4
            box(f, y - s // 2, y - s // 2 + s - 1, x - s // 2, x - s // 2 + s - 1, AMPS[n % 4])
            n += 1
    s = k + 2
    box(f, 0, s - 1, 0, s - 1, AMPS[0])
    box(f, 0, s - 1, w - s, w - 1, AMPS[1])
    box(f, h - s, h - 1, 0, s - 1, AMPS[2])
    box(f, h - s, h - 1, w - s, w - 1, AMPS[3])
    box(f, 12, 12 + k - 2, 30, 30 + k - 2, AMPS[3])          # k - 1 a side
    box(f, 42, 53, 20, 300, AMPS[2])                         # 12 x 281: long and thin after the erosion too
    return f


WIDE = "wide erosion"
for _fill in ("1", "0"):
    case(f"wide_9x9_fill{_fill}", WIDE, lambda: f_wide(96, 320, 9, 40), entries=("dim", "batch"), erode=ONES(9, 9), knobs={"LFDMI_SPARSE_ERODE_FILL": _fill},
         seams=[("row", 32), ("row", 64), ("col", 64), ("col", 128)], survivors=[(1, 1), (94, 318), (32, 64)], vanish=[(12, 19, 30, 37)], box_expected=True,
         expect=[dict(entry="dim", mode=0, front="wide", only_tiles=_fill == "1"), dict(entry="dim", mode=1, front="wide", only_tiles=False),
                 dict(entry="batch", mode=0, front="wide", only_tiles=_fill == "1")])
case("wide_7x7", WIDE, lambda: f_wide(72, 4096, 7, 41), entries=("dim",), erode=ONES(7, 7), seams=[("row", 32), ("row", 64), ("col", 64)],
     survivors=[(1, 1), (70, 4094), (32, 64)], vanish=[(12, 17, 30, 35)], expect=[dict(entry="dim", mode=0, front="wide", only_tiles=True)])
case("wide_7x7_keep", WIDE, lambda: f_wide(96, 320, 7, 42), entries=("dim",), erode=ONES(7, 7), seams=[("row", 32), ("col", 64)],
     survivors=[(1, 1), (32, 64)], vanish=[(12, 17, 30, 35)], expect=[dict(entry="dim", mode=0, front="band"), dict(entry="dim", mode=1, front="wide", only_tiles=False)])

# -- the workgroup of k_scan_fused --------------------------------------------------------------------------------------------

SCAN_H, SCAN_W = 416, 320                                    # wq = 5: word 2048 is word 3 of row 409


def f_scan():
    """Bit rows of five words: the second workgroup of the run scan starts at word 2048 = row 409, word 3 (column 192).  Thin
    horizontal bars on the rows around 409 lay edge runs across columns 191 / 192 (that boundary) and 127 / 128 (the one before)."""
    f = blank(SCAN_H, SCAN_W, 50)
    for k, y in enumerate(range(398, 416, 3)):
        box(f, y, y, 100, 230, AMPS[k % 4])
    box(f, 100, 104, 100, 140, AMPS[0])                     # wave boundary: word 512 = row 102, word 2
    return f


case("scan_workgroup", "workgroup of k_scan_fused", f_scan, entries=("bright",), seams=[("col", 192), ("col", 128)])
case("scan_workgroup_three_launches", "workgroup of k_scan_fused", f_scan, entries=("bright",), knobs={"LFDMI_SCAN_FUSED": "0"}, seams=[("col", 192)])

# -- the hole table of k_frame_contours ---------------------------------------------------------------------------------------

RING_LEN, RING_PITCH_Y, RING_PITCH_X = 22, 10, 36


def f_rings(n, h, w):
    """n bars of 1 x 22 pixels on a pitch of 10 x 36: dilated 4 x 4, each gets an edge ring of its own (25 x 4, length / width
    6.25) with one hole inside.  The ring's outer border and its hole border both pass lwTresh, so fit_minAreaRect accepts two
    rectangles per ring: a hole that is lost or handed to the wrong parent changes the count of accepted rectangles."""
    per = w // RING_PITCH_X
    f = blank(h, w, 60 + n % 7)
    for i in range(n):
        y, x = 4 + RING_PITCH_Y * (i // per), 6 + RING_PITCH_X * (i % per)
        f[y, x:x + RING_LEN] = AMPS[i % 4]
    return f


def f_island():
    """A thick hollow frame whose inner ring (203 x 21) is elongated, and an elongated island inside its hole."""
    f = blank(64, 256, 61)
    hollow(f, 8, 55, 16, 239, 12, AMPS[1])
    box(f, 30, 32, 60, 180, AMPS[3])                         # the island
    return f


HOLES = "hole table of k_frame_contours"
for _n, _h, _w in ((1023, 330, 1152), (1024, 330, 1152), (1025, 330, 1152), (1600, 400, 1440)):
    case(f"holes_{_n}", HOLES, (lambda n=_n, h=_h, w=_w: f_rings(n, h, w)), entries=("bright",), holes=_n, box_expected=True)
case("holes_island", HOLES, f_island, entries=("bright", "dim"), box_expected=True)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# what the label-table test (FRAME_RUNCAP) and the multi-frame tests run
RUNCAP_CASE = "tile_staircase"
SEQUENCE_CASES = (("wide_9x9_fill1", "dim"), ("tile_staircase", "dim"), ("reach_left", "bright"), ("band_5x5", "dim"))

NOT_REACHED = {
    "more than 128 tile columns": "64 x 129 = 8256 columns; check_shape refuses widths above 8191 (the cell bitmap holds 512 cells a band), so "
                                  "k_dilate_canny_w is reached through LFDMI_DC_TILELIST=0 only",
    "more than DCT_MAXBANDS bands": "16 x 513 = 8208 rows, refused by the same check",
    "FRAME_RUNCAP itself": "32768 runs need a frame far above the size limit of these cases; LFDMI_FRAME_RUNCAP lowers the table instead",
}
