"""Hand-made frames of the short-streak search, shared by tests/test_streak_ref.py (the restatement against answers worked by
hand) and tests/test_gpu_streak.py (the device against the restatement on the same frames).  All at bin 1 and L = 8, so the
working arrays are the flipped frames themselves.  BG and AMP are exact in 2^-20 units: g = 1024 and 65536."""
import numpy as np

import streak_ref as S

L = 8
BG, AMP = np.float32(1.0 / 1024), np.float32(1.0 / 16)
G_BG, G_AMP = 1024, 65536
SIGMA = 1.0 / 64
# off(i; s) for L = 8 and s = 0 .. 7, worked by hand: (2 s i + 7) / 14 rounded down; a negative slope negates the row
OFF8 = ((0, 0, 0, 0, 0, 0, 0, 0),
        (0, 0, 0, 0, 1, 1, 1, 1),
        (0, 0, 1, 1, 1, 1, 2, 2),
        (0, 0, 1, 1, 2, 2, 3, 3),
        (0, 1, 1, 2, 2, 3, 3, 4),
        (0, 1, 1, 2, 3, 4, 4, 5),
        (0, 1, 2, 3, 3, 4, 5, 6),
        (0, 1, 2, 3, 4, 5, 6, 7))


def put(frame, cells, value):
    """write ``value`` into the cells (j, i) of the flipped frame: (x, y) = (i, j) is buffer row H-1-j"""
    h = frame.shape[0]
    for j, i in cells:
        frame[h - 1 - j, i] = value
    return frame


def planted(q):
    """a 12 x 12 frame with one segment of AMP on a floor of BG -> (frame, (q, s, r0, c0))"""
    f = np.full((12, 12), BG, np.float32)
    if q == 0:
        s, r0, c0 = 3, 2, 1
        cells = [(r0 + OFF8[3][i], c0 + i) for i in range(L)]                     # Q[r][c] = G[r][c]
    else:
        s, r0, c0 = -2, 9, 3
        cells = [(c0 + i, r0 - OFF8[2][i]) for i in range(L)]                     # Q[r][c] = G[c][r]: cell (j, i) = (c, r)
    return put(f, cells, AMP), (q, s, r0, c0)


def diagonal():
    """the 45-degree tie: cells (k, k), k = 2 .. 9, are segment (s = 7, r0 = 2, c0 = 2) of both orientations"""
    f = np.full((12, 12), BG, np.float32)
    return put(f, [(k, k) for k in range(2, 10)], AMP), (0, 7, 2, 2)


def half_valid(n_valid):
    """a 2 x 8 frame whose only valid pixels are n_valid of the columns 0, 2, 5, 7 of row y = 0: at n_valid = 4 the one
    candidate is (q 0, s 0, r0 0, c0 0) with 2 N = L exactly; the sloped segments through the row take two of them"""
    f = np.zeros((2, 8), np.float32)
    return put(f, [(0, c) for c in (0, 2, 5, 7)[:n_valid]], AMP)


def blotted():
    return np.zeros((12, 12), np.float32)


def tall():
    """Wb = 5 < L <= Hb = 10: only q = 1 has segments; a column of AMP at x = 3, y = 1 .. 8"""
    f = np.full((10, 5), BG, np.float32)
    return put(f, [(j, 3) for j in range(1, 9)], AMP), (1, 0, 3, 1)


def expected(key, n_amp=L, n_bg=0, threshold=8.0):
    """the record of segment ``key`` whose cells are n_amp of AMP and n_bg of BG, from the definition's arithmetic"""
    q, s, r0, c0 = key
    n = n_amp + n_bg
    a = np.float32(float(n_amp * G_AMP + n_bg * G_BG) / 2.0 ** 20)
    snr = a / (np.float32(SIGMA) * np.sqrt(np.float32(n)))
    x1, y1, x2, y2, rho, theta = S.line_of(q, s, r0, c0, L, 1)
    return {"status": S.OK, "found": int(snr >= np.float32(threshold)), "q": q, "s": s, "r0": r0, "c0": c0, "n_pix": n, "sum": a,
            "snr": np.float32(snr), "x1": x1, "y1": y1, "x2": x2, "y2": y2, "rho": rho, "theta": theta}


def hand_frames():
    """[(name, frame)] of every hand case, for the device"""
    return [("planted-q0", planted(0)[0]), ("planted-q1", planted(1)[0]), ("diagonal", diagonal()[0]), ("half-4", half_valid(4)),
            ("half-3", half_valid(3)), ("blotted", blotted()), ("tall", tall()[0])]
