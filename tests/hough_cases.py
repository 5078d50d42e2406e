"""Named Hough cases and a plain restatement of what the host and the vote kernel decide for them.

``vote_shape`` restates the host side of a HoughLines launch (lfdmi.hip: lfdmi_hough_dims, ensure_tables, run_hough): the
accumulator dimensions, the float32 trig table, the angles per workgroup (AW = 1 << AWL), the slab row ranges, the chunk
lengths of the two lists, and how a list is cut into pieces.  ``chunk_list`` restates k_pixlist (runs of set pixels inside one
64-pixel word, cut every ``cm``), ``vote_model`` the per-chunk decision of k_hough_vote in float32 with one rounding per
operation.  Nothing here touches the device: tests/test_hough_cases_model.py checks on the CPU that every case of ``CASES``
lands on the path it is named for, tests/test_gpu_hough_shapes.py runs them on the device against the oracle.

Frames are thin (8 to 16 rows, or columns for the tall ones): the accumulator's size follows 2 (h + w) / rho, the oracle's
time h * w * numangle, so a 16 x 8183 frame reaches the slab widths of an 8 k x 8 k one at a thousandth of the work.
"""
import math

import numpy as np

VOTE_MAX_SLABS = 32
CHUNK_MAX = 64
MAX_ANGLES = 4096
LDS_BYTES = 152 * 1024
VOTE_WGS = 6144
MAGIC = np.float32(12582912.0)          # 1.5 * 2^23: bits(v + MAGIC) = 0x4B400000 + rint(v)
MAGIC_BITS = 0x4B400000
DEG = math.pi / 180

# LFDMI_COUNTERS slots (common.h) the tests read
C_NPIX_EQU, C_NPIX_BOX, C_NPEAK_EQU, C_NPEAK_BOX, C_OVERFLOW, C_NNZ_EQU, C_NPIXB_EQU, C_NPIXB_BOX = 3, 4, 5, 6, 7, 15, 18, 19


# ---- host restatement ---------------------------------------------------------------------------------------------------

def hough_dims(h, w, rho, theta):
    """lfdmi_hough_dims: numangle in double, numrho in float32 (an int divided by a float), both through lrint."""
    rho32, theta32 = np.float32(rho), np.float32(theta)
    na = int(np.rint(math.pi / float(theta32)))
    nr = int(np.rint(np.float32((w + h) * 2 + 1) / rho32))
    return na, nr


def trig_table(na, rho, theta):
    """ensure_tables / createTrigTable: the angle accumulated in float32, cos and sin in double times float32(1 / rho)."""
    irho = np.float32(1) / np.float32(rho)
    theta32 = np.float32(theta)
    ang = np.zeros(na, np.float32)
    a = np.float32(0)
    for n in range(na):
        ang[n] = a
        a = np.float32(a + theta32)
    ang = ang.astype(np.float64)
    return (np.cos(ang) * float(irho)).astype(np.float32), (np.sin(ang) * float(irho)).astype(np.float32)


def vote_shape(h, w, rho, theta=DEG, vote_split=4, n_img=1, nc=1, classes=True, balance=True, vote_wgs=VOTE_WGS):
    """What run_hough launches for nc frames of h x w: a dict with numangle, numrho, aw_log2, nslabs, per_slab, lo, hi,
    nbmax, cm_a, cm_b, cls_b, lmax, nsplit, balance, vsplit (the kernel's nsplit argument) and the table (cos, sin)."""
    na, nr = hough_dims(h, w, rho, theta)
    cos, sin = trig_table(na, rho, theta)
    c64, s64 = cos.astype(np.float64), sin.astype(np.float64)
    half = (nr - 1) // 2
    aw_log2 = 6
    while True:
        AW = 1 << aw_log2
        nslabs = (na + AW - 1) // AW
        per_slab = nslabs <= VOTE_MAX_SLABS
        lo, hi = [-half - 1] * VOTE_MAX_SLABS, [nr - half] * VOTE_MAX_SLABS        # bins -1 .. numrho: the guard cells belong to the range
        if per_slab:
            nbmax = 1
            for sl in range(nslabs):
                rmin = rmax = 0.0
                for n in range(sl * AW, min(na, (sl + 1) * AW)):
                    for cx in (0, w):
                        for cy in (0, h):
                            r = cx * c64[n] + cy * s64[n]
                            rmin, rmax = min(rmin, r), max(rmax, r)
                lo[sl] = max(-half - 1, math.floor(rmin) - 2)
                hi[sl] = min(nr - half, math.ceil(rmax) + 2)
                nbmax = max(nbmax, hi[sl] - lo[sl] + 1)
        else:
            nbmax = nr + 2
        if (nbmax << aw_log2) * 4 + 256 <= LDS_BYTES or aw_log2 == 0:
            break
        aw_log2 -= 1
    fits = (nbmax << aw_log2) * 4 + 256 <= LDS_BYTES
    AW = 1 << aw_log2
    lmax = []
    for sl in range(nslabs if per_slab else 1):
        sel = np.abs(cos[sl * AW:(sl + 1) * AW] if per_slab else cos).astype(np.float64)
        cmax = float(sel.max()) if len(sel) else 0.0
        l = math.floor(0.999 / cmax) + 1 if cmax > 0 else CHUNK_MAX
        lmax.append(int(min(CHUNK_MAX, max(1, l))))
    cm_a, cm_b, cls_b = min(lmax), 0, 0
    if per_slab and classes:
        mb = CHUNK_MAX + 1
        for sl in range(nslabs):
            if lmax[sl] >= 2 * cm_a:
                cls_b |= 1 << sl
                mb = min(mb, lmax[sl])
        if cls_b:
            cm_b = mb
    nsplit = 1
    while nsplit < vote_split and nslabs * n_img * nc * nsplit < vote_wgs:
        nsplit <<= 1
    bal = 1 if (balance and n_img == 2 and nsplit >= 2) else 0
    return dict(numangle=na, numrho=nr, aw_log2=aw_log2, subs=64 >> aw_log2, nslabs=nslabs, per_slab=per_slab, lo=lo[:min(nslabs, VOTE_MAX_SLABS)],
                hi=hi[:min(nslabs, VOTE_MAX_SLABS)], nbmax=nbmax, fits=fits, cm_a=cm_a, cm_b=cm_b, cls_b=cls_b, lmax=lmax, nsplit=nsplit,
                balance=bal, vsplit=2 * nsplit if bal else nsplit, cos=cos, sin=sin)


# ---- k_pixlist ----------------------------------------------------------------------------------------------------------

def chunk_list(img, cm, cross_word=False):
    """(y, x0, len) of every chunk of k_pixlist's list cut every ``cm``: the maximal stretches of set pixels of each 64-pixel
    word of each row.  cross_word (a WRONG restatement, for the tests that show the checks bite): a stretch that reaches the
    end of its word is measured on into the next word, whose own scan lists those pixels again."""
    m = np.asarray(img) != 0
    h, w = m.shape
    wq = (w + 63) >> 6
    pad = np.zeros((h, wq * 64 + 1), bool)
    pad[:, :w] = m
    ys, xs, ls = [], [], []
    for q in range(wq):
        blk = pad[:, q * 64:(q + 1) * 64]
        d = np.diff(np.concatenate([np.zeros((h, 1), np.int8), blk.astype(np.int8), np.zeros((h, 1), np.int8)], axis=1), axis=1)
        y0, b0 = np.nonzero(d == 1)
        y1, b1 = np.nonzero(d == -1)                 # same order: row-major, one end per start
        ln = b1 - b0
        if cross_word and len(ln):
            rest = pad[:, (q + 1) * 64:]
            ext = np.where(rest.all(axis=1), rest.shape[1], np.argmin(rest, axis=1)) if rest.shape[1] else np.zeros(h, int)
            ln = np.where(b1 == 64, ln + ext[y0], ln)
        ys.append(y0); xs.append(q * 64 + b0); ls.append(ln)
    y, x, ln = (np.concatenate(v).astype(np.int64) for v in (ys, xs, ls))
    pieces = (ln + cm - 1) // cm
    idx = np.repeat(np.arange(len(ln)), pieces)
    k = np.arange(len(idx)) - np.repeat(np.cumsum(pieces) - pieces, pieces)
    return y[idx], x[idx] + k * cm, np.minimum(cm, ln[idx] - k * cm)


# ---- k_hough_vote -------------------------------------------------------------------------------------------------------

def _bin(fx, ys, c, half_up=False):
    """LFD_BIN: rint(fl(fl(fx * c) + ys)) through the 1.5 * 2^23 addition (round-half-even), as an integer bin."""
    v = (fx * c).astype(np.float32) + ys
    if half_up:                                      # WRONG on purpose: floor(v + 1/2)
        return np.floor(v.astype(np.float64) + 0.5).astype(np.int64)
    return ((v + MAGIC).astype(np.float32).view(np.int32).astype(np.int64) - MAGIC_BITS)


OUTCOMES = ("one_bin", "estimate", "corr_high", "corr_low", "walk")


def vote_model(y, x0, L, cos, sin, wrong=None):
    """The decision of k_hough_vote for every (chunk, angle): float32, one rounding per operation, no fused multiply-add.
    Returns (b0, be, t, code, walk): the pixels of chunk i at angle n are t[i, n] in bin b0[i, n] and L[i] - t[i, n] in
    be[i, n], except where walk[i, n] (bins per pixel, see ``accumulate``); code indexes OUTCOMES.
    wrong: None, or one of the deliberately wrong restatements "t_off_by_one" (of the split; an estimate that is off by one is
    what the correction step is there to mend), "wrong_side" (the correction's step), "half_up" (every rounding to a bin)."""
    half_up = wrong == "half_up"
    fx0 = np.asarray(x0, np.float32)[:, None]
    fy = np.asarray(y, np.float32)[:, None]
    Li = np.asarray(L, np.int64)[:, None]
    fxe = (fx0 + (Li - 1).astype(np.float32)).astype(np.float32)
    c, s = cos[None, :].astype(np.float32), sin[None, :].astype(np.float32)
    with np.errstate(all="ignore"):
        inv_c = (np.float32(1) / c).astype(np.float32)
        half_s = np.where(c < 0, np.float32(-0.5), np.float32(0.5)).astype(np.float32)
        ys = (fy * s).astype(np.float32)
        w0 = ((fx0 * c).astype(np.float32) + ys).astype(np.float32)
        v0 = (w0 + MAGIC).astype(np.float32)
        b0, be = _bin(fx0, ys, c, half_up), _bin(fxe, ys, c, half_up)
        tf = ((((v0 - MAGIC).astype(np.float32) + half_s).astype(np.float32) - w0).astype(np.float32) * inv_c).astype(np.float32)
        tf = np.fmin(np.fmax(tf, np.float32(1)), (Li - 1).astype(np.float32))
        t = np.ceil(tf).astype(np.int64)
        fxb = (fx0 + t.astype(np.float32)).astype(np.float32)
        fxa = (fxb - np.float32(1)).astype(np.float32)
        ba, bb = _bin(fxa, ys, c, half_up), _bin(fxb, ys, c, half_up)
        one = b0 == be
        ok = one | ((ba == b0) & (bb == be))
        high = ba == be
        bc = _bin(np.where(high, fxa - np.float32(1), fxb + np.float32(1)).astype(np.float32), ys, c, half_up)
        step = np.where(high, -1, 1) * (-1 if wrong == "wrong_side" else 1)
        t2 = np.where(ok, t, t + step)
        ok2 = ok | np.where(high, bc == b0, (ba == b0) & (bb == b0) & (bc == be))
    code = np.where(one, 0, np.where(ok, 1, np.where(ok2, np.where(high, 2, 3), 4)))
    if wrong == "t_off_by_one":                        # the checks look at x0 + t - 1 and x0 + t, the split counts one pixel more
        t2 = np.where(ok & ~one, t + 1, t2)
    return b0, be, np.where(one, Li + 0 * t, t2), code, ~ok2


def accumulate(img, shape, wrong=None):
    """The accumulator (OpenCV layout, guard cells included) the device builds for ``img`` under launch shape ``shape``:
    every slab votes with the list of its class, every chunk with ``vote_model``.  wrong: see vote_model, plus
    "cross_word" (chunk_list) and "b_on_class_a" (a class-A slab votes with list B's longer chunks AND trusts the two-bin
    split without the exact checks, which only hold up to list A's length)."""
    na, nr, AW = shape["numangle"], shape["numrho"], 1 << shape["aw_log2"]
    half = (nr - 1) // 2
    acc = np.zeros((na + 2, nr + 2), np.int64)
    lists = {}
    for sl in range(shape["nslabs"]):
        cls = (shape["cls_b"] >> sl) & 1 if sl < VOTE_MAX_SLABS else 0
        cm = shape["cm_b"] if cls else shape["cm_a"]
        blind = False
        if wrong == "b_on_class_a" and not cls and shape["cm_b"] > 0:
            cm, blind = shape["cm_b"], True
        if cm not in lists:
            lists[cm] = chunk_list(img, cm, cross_word=wrong == "cross_word")
        y, x0, L = lists[cm]
        a0, a1 = sl * AW, min(na, (sl + 1) * AW)
        cos, sin = shape["cos"][a0:a1], shape["sin"][a0:a1]
        for k0 in range(0, len(y), 1 << 15):
            yy, xx, LL = y[k0:k0 + (1 << 15)], x0[k0:k0 + (1 << 15)], L[k0:k0 + (1 << 15)]
            b0, be, t, _, walk = vote_model(yy, xx, LL, cos, sin, wrong if wrong not in ("cross_word", "b_on_class_a") else None)
            if blind:
                walk = np.zeros_like(walk)
            col = np.broadcast_to(np.arange(a0, a1)[None, :] + 1, b0.shape)
            keep = ~walk
            rest = np.broadcast_to(LL[:, None], t.shape) - t
            np.add.at(acc, (col[keep], b0[keep] + half + 1), t[keep])
            np.add.at(acc, (col[keep], be[keep] + half + 1), rest[keep])
            for i, n in zip(*np.nonzero(walk)):                                  # the exact walk, pixel by pixel
                fx = np.arange(xx[i], xx[i] + LL[i]).astype(np.float32)
                ysn = np.float32(np.float32(yy[i]) * sin[n])
                r = _bin(fx, ysn, cos[n], wrong == "half_up")
                np.add.at(acc, (a0 + n + 1, r + half + 1), 1)
    return acc.astype(np.int32)


def outcome_counts(img, shape, limit=1 << 14):
    """How many (chunk, angle) pairs of ``img`` end in each of OUTCOMES (chunks longer than one pixel only, at most ``limit``
    of them per list, evenly spread: the model tests ask whether an outcome occurs, not how often)."""
    na, AW = shape["numangle"], 1 << shape["aw_log2"]
    out = dict.fromkeys(OUTCOMES, 0)
    lists = {}
    for sl in range(shape["nslabs"]):
        cls = (shape["cls_b"] >> sl) & 1 if sl < VOTE_MAX_SLABS else 0
        cm = shape["cm_b"] if cls else shape["cm_a"]
        if cm not in lists:
            y, x0, L = chunk_list(img, cm)
            sel = np.nonzero(L > 1)[0]
            if len(sel) > limit:
                sel = sel[np.linspace(0, len(sel) - 1, limit).astype(int)]
            lists[cm] = (y[sel], x0[sel], L[sel])
        y, x0, L = lists[cm]
        if not len(y):
            continue
        a0, a1 = sl * AW, min(na, (sl + 1) * AW)
        code = vote_model(y, x0, L, shape["cos"][a0:a1], shape["sin"][a0:a1])[3]
        for k, name in enumerate(OUTCOMES):
            out[name] += int((code == k).sum())
    return out


# ---- frames -------------------------------------------------------------------------------------------------------------

RUN_LENGTHS = range(1, 131)
RUN_OFFSETS = (0, 1, 31, 32, 62, 63)
RUN_PLAN = [(1 + (k * 37 % 780) % 130, RUN_OFFSETS[(k * 37 % 780) // 130]) for k in range(780)]   # every (length, bit offset) pair once, mixed


def f_full(h, w):
    return np.full((h, w), 255, np.uint8)


def f_empty(h, w):
    return np.zeros((h, w), np.uint8)


def f_rows(h, w):
    """full rows alternating with empty ones"""
    a = np.zeros((h, w), np.uint8)
    a[::2] = 255
    return a


def f_cols(h, w):
    """full columns 3 of 4 (the transposed frames' counterpart of f_rows: runs of three, every word full of them)"""
    a = np.full((h, w), 255, np.uint8)
    a[:, 3::4] = 0
    return a


def f_corners(h, w):
    a = np.zeros((h, w), np.uint8)
    a[0, 0] = a[0, w - 1] = a[h - 1, 0] = a[h - 1, w - 1] = 255
    return a


def f_corner(h, w):
    a = np.zeros((h, w), np.uint8)
    a[h - 1, w - 1] = 1
    return a


def runs_placed(h, w):
    """[(y, x, length)] of f_runs: RUN_PLAN laid out left to right, top to bottom, every run starting at its bit offset of a
    64-pixel word and at least one empty pixel after the run before it; runs that do not fit the width are left out."""
    out, y, x = [], 0, 0
    for ln, off in RUN_PLAN:
        if ln > w - 64:
            continue
        while y < h:
            xs = x + (off - x) % 64
            if xs + ln <= w:
                out.append((y, xs, ln))
                x = xs + ln + 1
                break
            y, x = y + 1, 0
        if y >= h:
            break
    return out


def f_runs(h, w):
    """runs of 1 .. 130 pixels starting at bits 0, 1, 31, 32, 62, 63 of a word (as many of RUN_PLAN as the frame holds); the
    last two rows hold runs that start at column 0 and runs that end at column w - 1"""
    a = np.zeros((h, w), np.uint8)
    for y, x, ln in runs_placed(h - 2, w):
        a[y, x:x + ln] = 200
    a[h - 2, :min(w, 130)] = 7
    a[h - 2, max(0, w - 65):] = 7
    a[h - 1, max(0, w - 130):] = 255
    return a


def f_edge(h, w):
    """runs that end at column w - 1 (row i: length 1, 2, 63, 64, 65, 100, 130, ...) and runs of the same lengths from column 0"""
    a = np.zeros((h, w), np.uint8)
    for i in range(h):
        ln = min(w // 2 - 1, (1, 2, 63, 64, 65, 100, 130, 129)[i % 8])
        a[i, w - ln:] = 255
        a[i, :ln] = 255
    return a


def f_rand(h, w):
    return ((np.random.default_rng(h * 10007 + w).random((h, w)) < 0.5) * 255).astype(np.uint8)


def transposed(f):
    def g(h, w):
        return np.ascontiguousarray(f(w, h).T)
    g.__doc__ = f"{f.__name__} of the w x h frame, transposed"
    return g


FRAMES = dict(full=f_full, empty=f_empty, rows=f_rows, cols=f_cols, corners=f_corners, corner=f_corner, runs=f_runs, edge=f_edge, rand=f_rand,
              edge_t=transposed(f_edge))


def frame(case):
    return FRAMES[case["frame"]](case["h"], case["w"])


# ---- cases --------------------------------------------------------------------------------------------------------------

def _case(name, frame_name, h, w, rho, div, **expect):
    """expect: what vote_shape must give for the case with the library's defaults (tests/test_hough_cases_model.py)"""
    return dict(name=name, frame=frame_name, h=h, w=w, rho=float(rho), div=div, theta=math.pi / div, expect=expect)


CASES = [
    # one case per slab width at rho = 1 (chunks of one or two pixels); 16 x 4848 is the last width with ranges, AW 8
    _case("aw32_r1_runs", "runs", 16, 620, 1, 180, awl=5, slabs=6, nbmax=631, cm_a=1, cm_b=2, cls_b=0b11110),
    _case("aw16_r1_rand", "rand", 16, 1300, 1, 180, awl=4, slabs=12, nbmax=1307, cm_a=1, cm_b=2, cls_b=0b11111111110),
    _case("aw8_r1_full", "full", 16, 4000, 1, 180, awl=3, slabs=23, nbmax=4007, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw8_r1_corner", "corner", 16, 4000, 1, 180, awl=3, slabs=23, nbmax=4007, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw8_r1_empty", "empty", 16, 4000, 1, 180, awl=3, slabs=23, nbmax=4007, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw8_r1_corners", "corners", 16, 4000, 1, 180, awl=3, slabs=23, nbmax=4007, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw8_r1_w64k", "edge", 16, 4032, 1, 180, awl=3, slabs=23, nbmax=4039, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw8_r1_w64k1", "edge", 16, 4033, 1, 180, awl=3, slabs=23, nbmax=4040, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw8_r1_w64k63", "edge", 16, 4031, 1, 180, awl=3, slabs=23, nbmax=4038, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw4_r1_t90", "runs", 16, 6000, 1, 90, awl=2, slabs=23, nbmax=6005, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("aw4_r1_window", "rows", 2, 4852, 1, 180, awl=2, slabs=45, nbmax=9711, cm_a=1, cm_b=0, cls_b=0b0),
    _case("aw2_r1_runs", "runs", 16, 4860, 1, 180, awl=1, slabs=90, nbmax=9755, cm_a=1, cm_b=0, cls_b=0b0),
    _case("aw2_r1_full", "full", 8, 8183, 1, 180, awl=1, slabs=90, nbmax=16385, cm_a=1, cm_b=0, cls_b=0b0),
    _case("w8191_r1", "edge", 16, 8191, 1, 180, awl=1, slabs=90, nbmax=16417, cm_a=1, cm_b=0, cls_b=0b0),
    _case("h8191_r1", "edge_t", 8191, 8, 1, 180, awl=1, slabs=90, nbmax=16401, cm_a=1, cm_b=0, cls_b=0b0),
    # the same widths with longer chunks: the two-bin split under SUBS > 1
    _case("aw32_r5_runs", "runs", 16, 4000, 5, 180, awl=5, slabs=6, nbmax=807, cm_a=5, cm_b=12, cls_b=0b100),
    _case("aw16_r5_runs", "runs", 16, 7000, 5, 180, awl=4, slabs=12, nbmax=1406, cm_a=5, cm_b=12, cls_b=0b1110000),
    _case("aw16_r5_w8191", "rows", 16, 8191, 5, 180, awl=4, slabs=12, nbmax=1644, cm_a=5, cm_b=12, cls_b=0b1110000),
    _case("aw8_r2_runs", "runs", 16, 8000, 2, 180, awl=3, slabs=23, nbmax=4006, cm_a=2, cm_b=4, cls_b=0b1111111110000000),
    _case("aw16_r4_full", "full", 16, 8191, 4, 180, awl=4, slabs=12, nbmax=2054, cm_a=4, cm_b=10, cls_b=0b1110000),
    _case("aw8_r3_runs", "runs", 16, 8191, 3, 180, awl=3, slabs=23, nbmax=2736, cm_a=3, cm_b=6, cls_b=0b111111110000000),
    # tall frames (w = 16 or 8): y carries the range, the slabs near 90 degrees the rows; the exact walk needs y s on an odd half bin
    # at the table's 90-degree entry (|cos| ~ 1e-6 / rho), which 16 rows never reach: y = 134 at rho 4, 268 at rho 8
    _case("t_aw8_r1", "rand", 4000, 16, 1, 180, awl=3, slabs=23, nbmax=4007, cm_a=1, cm_b=2, cls_b=0b1111111111111111111110),
    _case("t_aw16_r5", "full", 7000, 16, 5, 180, awl=4, slabs=12, nbmax=1407, cm_a=5, cm_b=12, cls_b=0b1110000),
    _case("t_aw2_r1", "cols", 4860, 16, 1, 180, awl=1, slabs=90, nbmax=9755, cm_a=1, cm_b=0, cls_b=0b0),
    _case("t_aw32_r4_walk", "full", 4000, 16, 4, 180, awl=5, slabs=6, nbmax=1006, cm_a=4, cm_b=10, cls_b=0b100),
    _case("t_aw16_r4_h8191", "full", 8191, 8, 4, 180, awl=4, slabs=12, nbmax=2054, cm_a=4, cm_b=10, cls_b=0b1110000),
    _case("t_aw64_r8_walk", "full", 1200, 16, 8, 180, awl=6, slabs=3, nbmax=158, cm_a=8, cm_b=0, cls_b=0b0),
    # rhos: powers of two (x cos / rho exactly on r + 1/2 at theta = 0), CHUNK_MAX (rho >= 64), odd, class B at rho 20.  The *_thin cases
    # have fewer rows than rho: x cos / rho alone rounds one bin past (numrho - 1) / 2, into OpenCV's guard cells
    _case("r2", "runs", 16, 4000, 2, 180, awl=4, slabs=12, nbmax=2006, cm_a=2, cm_b=4, cls_b=0b11110000),
    _case("r4", "runs", 16, 4000, 4, 180, awl=5, slabs=6, nbmax=1007, cm_a=4, cm_b=10, cls_b=0b100),
    _case("r8", "runs", 16, 4000, 8, 180, awl=6, slabs=3, nbmax=527, cm_a=8, cm_b=0, cls_b=0b0),
    _case("r16", "runs", 16, 4000, 16, 180, awl=6, slabs=3, nbmax=267, cm_a=16, cm_b=0, cls_b=0b0),
    _case("r32_thin", "full", 16, 1000, 32, 180, awl=6, slabs=3, nbmax=39, cm_a=32, cm_b=0, cls_b=0b0),
    _case("r64_thin", "runs", 16, 1000, 64, 180, awl=6, slabs=3, nbmax=23, cm_a=64, cm_b=0, cls_b=0b0),
    _case("r100_thin", "runs", 16, 4000, 100, 180, awl=6, slabs=3, nbmax=48, cm_a=64, cm_b=0, cls_b=0b0),
    _case("r100_thin_full", "full", 16, 4000, 100, 180, awl=6, slabs=3, nbmax=48, cm_a=64, cm_b=0, cls_b=0b0),
    _case("r3", "runs", 16, 4000, 3, 180, awl=4, slabs=12, nbmax=1340, cm_a=3, cm_b=7, cls_b=0b1110000),
    _case("r20_class_b", "runs", 16, 2000, 20, 360, awl=6, slabs=6, nbmax=105, cm_a=20, cm_b=46, cls_b=0b100),
    _case("r64_thin_full", "full", 16, 1000, 64, 180, awl=6, slabs=3, nbmax=23, cm_a=64, cm_b=0, cls_b=0b0),
    _case("r64_tall", "runs", 72, 1000, 64, 180, awl=6, slabs=3, nbmax=23, cm_a=64, cm_b=0, cls_b=0b0),
    # other numangle: 32 slabs is the last count with ranges
    _case("th90", "rand", 64, 64, 1, 90, awl=6, slabs=2, nbmax=134, cm_a=1, cm_b=0, cls_b=0b0),
    _case("th360", "rand", 64, 128, 1, 360, awl=6, slabs=6, nbmax=176, cm_a=1, cm_b=2, cls_b=0b11110),
    _case("th1024", "rand", 64, 256, 1, 1024, awl=6, slabs=16, nbmax=281, cm_a=1, cm_b=2, cls_b=0b111111111111110),
    _case("th2048_32slabs", "rand", 64, 256, 1, 2048, awl=6, slabs=32, nbmax=276, cm_a=1, cm_b=2, cls_b=0b1111111111111111111111111111110),
    _case("th4096_64slabs", "rand", 64, 64, 1, 4096, awl=6, slabs=64, nbmax=259, cm_a=1, cm_b=0, cls_b=0b0),
    _case("th4096_aw32", "runs", 64, 256, 1, 4096, awl=5, slabs=128, nbmax=643, cm_a=1, cm_b=0, cls_b=0b0),
    _case("th1024_r4", "full", 64, 256, 4, 1024, awl=6, slabs=16, nbmax=75, cm_a=4, cm_b=8, cls_b=0b11111100000),
]
BY_NAME = {c["name"]: c for c in CASES}

# launch variants every case runs under: (id, environment); the default cuts a single frame's list into four pieces
VARIANTS = [("default", {}), ("split1", {"LFDMI_VOTE_SPLIT": "1"}), ("split2", {"LFDMI_VOTE_SPLIT": "2"}), ("split8", {"LFDMI_VOTE_SPLIT": "8"}),
            ("split16", {"LFDMI_VOTE_SPLIT": "16"}), ("classes0", {"LFDMI_VOTE_CLASSES": "0"})]


def variant_shape(case, env, **kw):
    return vote_shape(case["h"], case["w"], case["rho"], case["theta"], vote_split=int(env.get("LFDMI_VOTE_SPLIT", 4)),
                      classes=env.get("LFDMI_VOTE_CLASSES", "1") != "0", balance=env.get("LFDMI_VOTE_BALANCE", "1") != "0", **kw)


def ctx_dims(case):
    """(max_h, max_w) of a context whose accumulator storage (sized for theta = pi / 180 at rho = 1) holds the case's"""
    na, nr = hough_dims(case["h"], case["w"], case["rho"], case["theta"])
    need = -(-(na + 2) * (nr + 2) // 182)                  # (numrho + 2) of the context's own frame size at rho 1
    w = max(case["w"], -(-(need - 3) // 2) - case["h"])
    assert w <= 8191, case["name"]
    return case["h"], w


# ---- frames for the two-image path (process_bright / process_dim: HoughLines on the equalised image and on the box image) ----

def p_noise_streak():
    """noise everywhere and one streak: the equalised image's list is about a hundred times the box image's"""
    h, w = 300, 400
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.random.default_rng(3).normal(0.3, 0.8, (h, w)).astype(np.float32)
    a[np.abs(yy - (0.4 * xx + 20)) < 2.0] += 60.0
    return a


def p_thin():
    """a thin line on an empty frame (wide enough to outlive the dim pass's 3 x 3 erosion): both lists about equally long at rho 20"""
    h, w = 200, 333
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w), np.float32)
    a[np.abs(yy - (-0.5 * xx + 180)) < 2.0] = 50.0
    return a


def p_bar():
    """a bar on an empty frame: the box image is the outline of one thin rectangle"""
    h, w = 128, 256
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w), np.float32)
    a[np.abs(yy - (0.3 * xx + 30)) < 6.0] = 80.0
    return a


PASS_FRAMES = dict(noise_streak=p_noise_streak, thin=p_thin, bar=p_bar)
PASS_VARIANTS = [(s, b) for s in ("2", "4", "16") for b in ("0", "1")]     # (LFDMI_VOTE_SPLIT, LFDMI_VOTE_BALANCE)
