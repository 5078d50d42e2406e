"""The frame previews of include/lfdmi.h (frame previews, steps 1 - 6) restated in numpy: the device matches every byte, every
int64 cell and every record field (tests/test_gpu_preview*.py); the CPU tests work its answers by hand and measure the defaults."""
import numpy as np

FRAME_DTYPE = np.dtype([("status", "<i4"), ("n_cells", "<i4"), ("n_empty", "<i4"), ("pad", "<i4"),
                        ("lo", "<i8"), ("hi", "<i8"), ("lo_f", "<f8"), ("hi_f", "<f8")])
OK, FLAT, EMPTY = 0, 1, 2
RANK, GIVEN = 0, 1
LUT = 4096
BINS = (1, 2, 4, 8, 16)
EMPTY_CELL = -2 ** 63
CLAMP = 16777216.0          # 2^24
SCALE = 1073741824.0        # 2^30
DEFAULTS = {"bin": 4, "mode": RANK, "lo_ppm": 10000, "hi_ppm": 995000}


def fixed(v):
    """step 2: (valid, q) of float32 values; q is 0 where the pixel is not valid"""
    v = np.asarray(v, np.float32)
    valid = np.isfinite(v)
    c = np.clip(np.where(valid, v, np.float32(0)).astype(np.float64), -CLAMP, CLAMP) * SCALE
    return valid, np.rint(c).astype(np.int64)


def given_fixed(x):
    """step 4, GIVEN: a finite double limit as an integer"""
    return int(np.rint(min(max(float(x), -CLAMP), CLAMP) * SCALE))


def trunc_div(q, c):
    """q / c as C divides int64 (towards zero); c > 0"""
    return np.sign(q) * (np.abs(q) // c)


def cells(frame, bin):
    """steps 1 and 3: the int64 cell plane (Hp, Wp) of one native float32 frame in buffer-row order; EMPTY_CELL where no pixel is valid"""
    b = int(bin)
    x = np.asarray(frame, np.float32)[::-1]                 # the flipped frame
    h, w = x.shape
    hp, wp = -(-h // b), -(-w // b)
    valid, q = fixed(x)
    Q = np.zeros((hp * b, wp * b), np.int64)
    C = np.zeros((hp * b, wp * b), np.int64)
    Q[:h, :w], C[:h, :w] = q, valid
    Q = Q.reshape(hp, b, wp, b).sum(axis=(1, 3))
    C = C.reshape(hp, b, wp, b).sum(axis=(1, 3))
    m = trunc_div(Q, np.maximum(C, 1))
    return np.where(C == 0, np.int64(EMPTY_CELL), m)


def rank_limits(m, lo_ppm, hi_ppm):
    """step 4, RANK: (M, lo, hi) of a cell plane; lo = hi = 0 with M == 0"""
    v = np.sort(m[m != EMPTY_CELL].reshape(-1))
    M = len(v)
    if M == 0:
        return 0, 0, 0
    return M, int(v[(int(lo_ppm) * (M - 1)) // 1000000]), int(v[(int(hi_ppm) * (M - 1)) // 1000000])


def levels(m, lo, hi):
    """step 5: k of every cell of an OK frame (EMPTY cells: 0, not looked up)"""
    d = np.clip(m, lo, hi) - np.int64(lo)
    k = ((d.astype(np.float64) / float(hi - lo)) * 4095.0).astype(np.int64)
    return np.where(m == EMPTY_CELL, 0, k)


def render(m, status, lo, hi, lut):
    """steps 4 - 5: the bytes of a cell plane"""
    if status != OK:
        return np.zeros(m.shape, np.uint8)
    return np.where(m == EMPTY_CELL, np.uint8(0), np.asarray(lut, np.uint8)[levels(m, lo, hi)]).astype(np.uint8)


def frame_previews(frames, lut, bin=4, mode=RANK, lo_ppm=10000, hi_ppm=995000, limits=None):
    """The whole call: (uint8 [n, Hp, Wp], int64 cells [n, Hp, Wp], FRAME_DTYPE records [n]).  frames: [n, h, w] float32 (native
    or big-endian: numpy converts); limits: [n, 2] doubles with mode GIVEN."""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    b = int(bin)
    hp, wp = -(-h // b), -(-w // b)
    out = np.zeros((n, hp, wp), np.uint8)
    cel = np.zeros((n, hp, wp), np.int64)
    rec = np.zeros(n, FRAME_DTYPE)
    if mode == GIVEN:
        limits = np.broadcast_to(np.asarray(limits, np.float64), (n, 2))
    for i in range(n):
        m = cells(frames[i].astype(np.float32), b)
        M, lo, hi = rank_limits(m, lo_ppm, hi_ppm)
        if mode == GIVEN:
            lo, hi = given_fixed(limits[i, 0]), given_fixed(limits[i, 1])
        status = EMPTY if M == 0 else (OK if hi > lo else FLAT)
        cel[i] = m
        out[i] = render(m, status, lo, hi, lut)
        rec[i] = (status, M, hp * wp - M, 0, lo, hi, float(lo) * 2.0 ** -30, float(hi) * 2.0 ** -30)
    return out, cel, rec
