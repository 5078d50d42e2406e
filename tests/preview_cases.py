"""Hand-worked frames for the frame previews: each case names what it holds and carries the answer worked by hand, which
tests/test_preview_ref.py asks of the restatement and tests/test_gpu_preview_edges.py of the device.  A pixel of k * 2^-30 enters
as the integer k, so the arithmetic below is the arithmetic of the definition."""
import numpy as np

import preview_ref as R

U = np.float32(2.0 ** -30)          # one unit of q
E = R.EMPTY_CELL
NAN, INF = np.float32("nan"), np.float32("inf")
_K = np.arange(R.LUT)
TEST_LUT = ((_K // 16 + _K * 3 + 3) % 256).astype(np.uint8)   # lut[0] = 3 (not an EMPTY cell's 0), lut[2047] = 127, lut[4095] = 255


def _units(rows):
    return (np.array(rows, np.float32) * U).astype(np.float32)


class Case:
    def __init__(self, frames, params, cells=None, out=None, records=None, limits=None):
        frames = np.asarray(frames, np.float32)
        self.frames = frames[None] if frames.ndim == 2 else frames
        self.params, self.limits = dict(params), limits
        self.cells = None if cells is None else np.array(cells, np.int64).reshape((len(self.frames),) + np.shape(cells)[-2:])
        self.out = None if out is None else np.array(out, np.uint8).reshape(self.cells.shape)
        self.records = records          # [(status, n_cells, n_empty, lo, hi)] per frame

    def kwargs(self):
        kw = dict(self.params)
        if self.limits is not None:
            kw["limits"] = self.limits
        return kw


def _cases():
    c = {}
    full = {"lo_ppm": 0, "hi_ppm": 1000000}
    # q = -1 and -2: Q = -3, n = 2, and C's division gives -1 (floor would give -2).  M = 1: FLAT
    c["truncating_division"] = Case(_units([[-1, -2]]), {"bin": 2, **full}, cells=[[-1]], out=[[0]], records=[(R.FLAT, 1, 0, -1, -1)])
    # 3 x 5 at bin 2: flipped rows [10..14], [5..9], [0..4]; the last row and column of cells are partial
    #   (10+11+5+6)/4 = 8   (12+13+7+8)/4 = 10   (14+9)/2 = 11 (11.5 truncated)
    #   (0+1)/2 = 0         (2+3)/2 = 2          4/1 = 4
    # lo = 0, hi = 11: k = (int)(m / 11 * 4095) = 2978, 3722, 4095 / 0, 744, 1489
    k = [[2978, 3722, 4095], [0, 744, 1489]]
    c["partial_last_row_and_column"] = Case(_units(np.arange(15).reshape(3, 5)), {"bin": 2, **full},
                                            cells=[[8, 10, 11], [0, 2, 4]], out=TEST_LUT[np.array(k)], records=[(R.OK, 6, 0, 0, 11)])
    # 2 x 4 at bin 2: cell 0 holds NaN, 3, inf, 4 -> Q = 7, n = 2, m = 3; cell 1 holds no finite pixel: EMPTY.  M = 1: FLAT
    f = np.array([[NAN, 3 * U, NAN, -INF], [INF, 4 * U, INF, NAN]], np.float32)
    c["some_and_all_pixels_not_finite"] = Case(f, {"bin": 2, **full}, cells=[[3, E]], out=[[0, 0]], records=[(R.FLAT, 1, 1, 3, 3)])
    # the clamp: 3e7 > 2^24 enters as 2^54, 2^24 itself too, +-inf are not valid.  lo = -2^54, hi = 2^54: k = 4095, 0, 4095, 0 (EMPTY), 0
    f = np.array([[3e7, -3e7, 16777216.0, INF, -INF]], np.float32)
    c["clamp_and_infinities"] = Case(f, {"bin": 1, **full}, cells=[[2 ** 54, -2 ** 54, 2 ** 54, E, E]],
                                     out=[[TEST_LUT[4095], TEST_LUT[0], TEST_LUT[4095], 0, 0]], records=[(R.OK, 3, 2, -2 ** 54, 2 ** 54)])
    # ranks at ppm 0 and 1000000: the smallest and the largest of 5, 1, 4, 2, 3.  k = 4095, 0, 3071, 1023, 2047
    c["ranks_at_the_ends"] = Case(_units([[5, 1, 4, 2, 3]]), {"bin": 1, **full}, cells=[[5, 1, 4, 2, 3]],
                                  out=TEST_LUT[np.array([[4095, 0, 3071, 1023, 2047]])], records=[(R.OK, 5, 0, 1, 5)])
    # ranks inside: (250000 * 4) / 1000000 = 1 -> 2; (999999 * 4) / 1000000 = 3 -> 4.  d = 2, 0, 2, 0, 1 of r = 2
    c["ranks_inside"] = Case(_units([[5, 1, 4, 2, 3]]), {"bin": 1, "lo_ppm": 250000, "hi_ppm": 999999}, cells=[[5, 1, 4, 2, 3]],
                             out=TEST_LUT[np.array([[4095, 0, 4095, 0, 2047]])], records=[(R.OK, 5, 0, 2, 4)])
    # M == 1: both ranks are the one cell: FLAT
    c["one_cell"] = Case(_units([[7]]), {"bin": 4}, cells=[[7]], out=[[0]], records=[(R.FLAT, 1, 0, 7, 7)])
    # a constant frame is FLAT, a frame without a finite pixel EMPTY (lo = hi = 0), the frame between them is ordinary
    f = np.stack([np.full((2, 2), 9 * U, np.float32), np.full((2, 2), NAN, np.float32), _units([[0, 1], [2, 4]])])
    c["flat_empty_ordinary"] = Case(f, {"bin": 1, **full}, cells=[[[9, 9], [9, 9]], [[E, E], [E, E]], [[2, 4], [0, 1]]],
                                    out=[[[0, 0], [0, 0]], [[0, 0], [0, 0]], TEST_LUT[np.array([[2047, 4095], [0, 1023]])]],
                                    records=[(R.FLAT, 4, 0, 9, 9), (R.EMPTY, 0, 4, 0, 0), (R.OK, 4, 0, 0, 4)])
    # k at both ends of the table and in its middle: 0, (int)(0.5 * 4095) = 2047, 4095
    c["both_ends_of_the_table"] = Case(_units([[0, 1, 2]]), {"bin": 1, **full}, cells=[[0, 1, 2]],
                                       out=[[TEST_LUT[0], TEST_LUT[2047], TEST_LUT[4095]]], records=[(R.OK, 3, 0, 0, 2)])
    # GIVEN limits 0 and 4 units: -5 clamps to k = 0, 1 gives (int)(0.25 * 4095) = 1023, 9 clamps to 4095
    c["given_limits"] = Case(_units([[-5, 1, 9]]), {"bin": 1, "mode": R.GIVEN}, limits=np.array([[0.0, 4.0 * 2.0 ** -30]]),
                             cells=[[-5, 1, 9]], out=[[TEST_LUT[0], TEST_LUT[1023], TEST_LUT[4095]]], records=[(R.OK, 3, 0, 0, 4)])
    # GIVEN limits the wrong way round: FLAT; and on a frame without a finite pixel: EMPTY, which keeps them
    f = np.stack([_units([[1, 2]]), np.full((1, 2), NAN, np.float32)])
    c["given_flat_and_empty"] = Case(f, {"bin": 1, "mode": R.GIVEN}, limits=np.array([[3.0, 1.0], [1.0, 3.0]]) * 2.0 ** -30,
                                     cells=[[[1, 2]], [[E, E]]], out=[[[0, 0]], [[0, 0]]],
                                     records=[(R.FLAT, 2, 0, 3, 1), (R.EMPTY, 0, 2, 1, 3)])
    # ties: 50 cells of 0 and 50 of 1; (500000 * 99) / 1000000 = 49 is the last 0 and (510000 * 99) / 1000000 = 50 the first 1
    f = _units(np.r_[np.zeros(50), np.ones(50)].reshape(10, 10))
    k = np.where(f[::-1] > 0, 4095, 0)
    c["tie_on_the_boundary"] = Case(f, {"bin": 1, "lo_ppm": 500000, "hi_ppm": 510000}, cells=(f[::-1] > 0).astype(np.int64),
                                    out=TEST_LUT[k], records=[(R.OK, 100, 0, 0, 1)])
    # ... and one rank lower on both sides the limits are equal: FLAT
    c["tie_below_the_boundary"] = Case(f, {"bin": 1, "lo_ppm": 490000, "hi_ppm": 500000}, cells=(f[::-1] > 0).astype(np.int64),
                                       out=np.zeros((10, 10)), records=[(R.FLAT, 100, 0, 0, 0)])
    return c


CASES = _cases()
NAMES = tuple(CASES)


def check(name, out, cells, rec):
    """the hand-worked answer of a case against what a restatement or the device returned"""
    c = CASES[name]
    assert cells.dtype == np.int64 and out.dtype == np.uint8 and rec.dtype == R.FRAME_DTYPE, name
    assert cells.tolist() == c.cells.tolist(), (name, cells, c.cells)
    assert out.tolist() == c.out.tolist(), (name, out, c.out)
    for i, (status, n_cells, n_empty, lo, hi) in enumerate(c.records):
        r = rec[i]
        assert (int(r["status"]), int(r["n_cells"]), int(r["n_empty"]), int(r["pad"]), int(r["lo"]), int(r["hi"])) == \
            (status, n_cells, n_empty, 0, lo, hi), (name, i, r)
        assert float(r["lo_f"]) == lo * 2.0 ** -30 and float(r["hi_f"]) == hi * 2.0 ** -30, (name, i, r)
