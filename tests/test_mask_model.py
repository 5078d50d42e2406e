"""The trail masks' definition (include/lfdmi.h: trail masks) as tests/mask_ref.py restates it, without a GPU: known answers, the
half-width rule, how much of an injected trail's flux a mask holds, the packed form, the segment builders and the masks.txt row."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import mask_ref as MR  # noqa: E402

from lfd_amd import _native, masks  # noqa: E402


def test_the_layouts_agree():
    import ctypes as C
    assert MR.SEGMENT_DTYPE == _native.MASK_SEGMENT_DTYPE and MR.SEGMENT_DTYPE.itemsize == 64 == C.sizeof(_native.MaskSegment)
    assert [n for n, *_ in _native.MaskSegment._fields_] == list(MR.SEGMENT_DTYPE.names)
    for name, _ in _native.MaskSegment._fields_:
        assert getattr(_native.MaskSegment, name).offset == MR.SEGMENT_DTYPE.fields[name][1], name
    assert MR.STAT_DTYPE == _native.MASK_STAT_DTYPE and MR.STAT_DTYPE.itemsize == 8
    assert C.sizeof(_native.MaskParamsStruct) == 8
    assert (MR.OK, MR.BAD_SEGMENT, MR.EMPTY) == (_native.MASK_OK, _native.MASK_BAD_SEGMENT, _native.MASK_EMPTY)
    assert [_native.MASK_FILLS[k] for k in MR.FILLS] == [0, 1, 2, 3]
    p = _native.make_mask_params()
    assert (p.fill_mode, p.clear) == (_native.MASK_FILL_NONE, 1)
    assert _native.make_mask_params(fill_mode="NaN", clear=0).fill_mode == _native.MASK_FILL_NAN
    with pytest.raises(TypeError) as e:
        _native.make_mask_params(no_such_field=1)
    assert str(e.value) == "unknown mask parameter 'no_such_field'"
    with pytest.raises(ValueError):
        _native.make_mask_params(fill_mode="median")


def test_a_horizontal_segment_masks_its_rows_and_columns():
    H, W = 32, 40
    s = MR.segment(0, 5.0, 10.0, 20.0, 10.0, half=2.0, cap=0.0)
    mask, stats, counts = MR.mask_trails([s], (1, H, W))
    want = np.zeros((H, W), np.uint8)
    want[H - 1 - 12:H - 1 - 8 + 1, 5:21] = 1                       # flipped rows 8 .. 12 are buffer rows H-1-12 .. H-1-8
    assert np.array_equal(mask[0], want)
    assert tuple(stats[0]) == (MR.OK, 80) and counts.tolist() == [80]
    # the same segment from the other end, and with a cap of 3 px
    mask2, stats2, _ = MR.mask_trails([MR.segment(0, 20.0, 10.0, 5.0, 10.0, half=2.0)], (1, H, W))
    assert np.array_equal(mask2, mask)
    mask3, stats3, _ = MR.mask_trails([MR.segment(0, 5.0, 10.0, 20.0, 10.0, half=2.0, cap=3.0)], (1, H, W))
    want[H - 1 - 12:H - 1 - 8 + 1, 2:24] = 1
    assert np.array_equal(mask3[0], want) and int(stats3[0]["n_pix"]) == 5 * 22


def test_half_zero_masks_only_centres_on_the_line():
    H, W = 16, 24
    mask, stats, _ = MR.mask_trails([MR.segment(0, 2.0, 3.0, 9.0, 3.0, half=0.0)], (1, H, W))
    assert int(stats[0]["n_pix"]) == 8 and mask[0, H - 1 - 3, 2:10].all() and int(mask.sum()) == 8
    # the diagonal through integer points: exactly those
    mask, stats, _ = MR.mask_trails([MR.segment(0, 1.0, 1.0, 6.0, 6.0, half=0.0)], (1, H, W))
    assert sorted(zip(*np.nonzero(mask[0]))) == [(H - 1 - k, k) for k in range(6, 0, -1)]
    # a line between the pixel centres: none, and the record says so
    mask, stats, _ = MR.mask_trails([MR.segment(0, 2.0, 3.5, 9.0, 3.5, half=0.0)], (1, H, W))
    assert not mask.any() and tuple(stats[0]) == (MR.EMPTY, 0)


def test_an_infinite_cap_reaches_both_edges():
    H, W = 20, 50
    mask, stats, _ = MR.mask_trails([MR.segment(0, 20.0, 7.0, 22.0, 7.0, half=1.0, cap=np.inf)], (1, H, W))
    assert mask[0, H - 1 - 8:H - 1 - 6 + 1, :].all() and int(stats[0]["n_pix"]) == 3 * W == int(mask.sum())
    mask, stats, _ = MR.mask_trails([MR.segment(0, 5.0, 9.0, 5.0, 8.0, half=0.5, cap=np.inf)], (1, H, W))
    assert mask[0, :, 5].all() and int(mask.sum()) == H


def test_crossing_segments_or_their_bits_and_value_fill_takes_the_lower_index():
    H, W = 40, 40
    segs = [MR.segment(0, 0.0, 20.0, 39.0, 20.0, half=2.0, bits=1, fill=7.0),
            MR.segment(0, 20.0, 0.0, 20.0, 39.0, half=2.0, bits=2, fill=-3.5)]
    frames = np.full((1, H, W), 0.25, np.float32)
    mask, stats, counts = MR.mask_trails(segs, (1, H, W), frames=frames, fill="value")
    cross = mask[0, H - 1 - 22:H - 1 - 18 + 1, 18:23]
    assert (cross == 3).all() and int((mask == 3).sum()) == 25
    assert (frames[0, H - 1 - 22:H - 1 - 18 + 1, 18:23] == 7.0).all()
    assert set(np.unique(frames)) == {np.float32(0.25), np.float32(7.0), np.float32(-3.5)}
    assert stats["n_pix"].tolist() == [200, 200] and counts.tolist() == [375]
    # the other order: the crossing takes the other value, the mask is the same
    frames2 = np.full((1, H, W), 0.25, np.float32)
    mask2, _, _ = MR.mask_trails(segs[::-1], (1, H, W), frames=frames2, fill="value")
    assert np.array_equal(mask2, mask) and (frames2[0, H - 1 - 22:H - 1 - 18 + 1, 18:23] == -3.5).all()


def test_outside_and_bad_segments_touch_nothing():
    H, W = 24, 30
    rng = np.random.default_rng(1)
    frames = rng.normal(0, 1, (1, H, W)).astype(np.float32)
    frames[0, 3, 4] = np.float32(-0.0)
    frames.view(np.uint32)[0, 5, 6] = 0x7FC12345
    before = frames.copy()
    bad = [MR.segment(0, 100.0, 100.0, 200.0, 150.0, half=3.0),                   # wholly outside: EMPTY
           MR.segment(0, 5.0, 5.0, 5.0, 5.0, half=3.0),                           # zero length
           MR.segment(0, np.nan, 5.0, 9.0, 5.0, half=3.0),
           MR.segment(0, 5.0, np.inf, 9.0, 5.0, half=3.0),
           MR.segment(0, 2e6, 5.0, 9.0, 5.0, half=3.0),
           MR.segment(0, 1.0, 5.0, 9.0, 5.0, half=-1.0),
           MR.segment(0, 1.0, 5.0, 9.0, 5.0, half=np.inf),
           MR.segment(0, 1.0, 5.0, 9.0, 5.0, half=np.nan),
           MR.segment(0, 1.0, 5.0, 9.0, 5.0, half=1.0, cap=-1.0),
           MR.segment(0, 1.0, 5.0, 9.0, 5.0, half=1.0, cap=np.nan)]
    mask, stats, counts = MR.mask_trails(bad, (1, H, W), frames=frames, fill="nan")
    assert not mask.any() and counts.tolist() == [0]
    assert stats["status"].tolist() == [MR.EMPTY] + [MR.BAD_SEGMENT] * 9 and not stats["n_pix"].any()
    assert np.array_equal(frames.view(np.uint32), before.view(np.uint32))
    # a coordinate of exactly 1e6 is good
    assert MR.geometry(MR.segment(0, 1e6, 5.0, 9.0, 5.0, half=1.0)) is not None


def test_fills_and_clear():
    H, W = 12, 16
    s = [MR.segment(0, 2.0, 4.0, 9.0, 4.0, half=1.0, bits=4)]
    for fill, want in (("zero", 0x00000000), ("nan", 0x7FC00000)):
        frames = np.full((1, H, W), -1.5, np.float32)
        mask, _, _ = MR.mask_trails(s, (1, H, W), frames=frames, fill=fill)
        assert (frames.view(np.uint32)[mask != 0] == want).all() and (frames[mask == 0] == -1.5).all()
    old = np.full((1, H, W), 0x81, np.uint8)
    kept, _, _ = MR.mask_trails(s, (1, H, W), mask=old.copy(), clear=False)
    assert set(np.unique(kept)) == {0x81, 0x85} and int((kept == 0x85).sum()) == 24
    cleared, _, _ = MR.mask_trails(s, (1, H, W), mask=old.copy(), clear=True)
    assert set(np.unique(cleared)) == {0, 4}


def test_half_width():
    assert masks.half_width(4.71) == max(4.0, 2.0 * 4.71 / 2.0) + 2.0 == 6.71
    assert masks.half_width(1.0) == 6.0                                           # min_half
    assert masks.half_width(10.0, k_fwhm=3.0, grow=1.0) == 16.0
    assert masks.half_width(2.0, min_half=0.5, grow=0.0) == 2.0
    for fwhm in (float("nan"), 0.0, -3.0):
        assert masks.half_width(fwhm) == 10.0
        assert masks.half_width(fwhm, default_half=5.0, grow=0.5) == 5.5


def test_the_mask_holds_the_injected_flux():
    """A Gaussian trail of sigma 2 px: the band |u| <= half holds erf(half / (2 sqrt 2)) of its flux; a mask of pixel centres
    holds every pixel that lies wholly within half - 1/2 px of the line along either axis, so at least the band of half - 1."""
    from lfd_amd import inject, synth
    shape = (372, 512)
    base = synth.make_frame(3, shape, with_catalog=False)[0]
    table, step = inject.gaussian_table(2.0)
    table = inject.normalise_peak(table).astype(np.float32)
    theta = 1.1
    rho = 256.0 * math.cos(theta) + 186.0 * math.sin(theta)
    tr = np.array([IR.trail(0, 0, rho, theta, amplitude=1.0)], IR.TRAIL_DTYPE)
    after = IR.inject(base[None].copy(), tr, table, step, 4)[0]
    flux = after.astype(np.float64) - base.astype(np.float64)
    c, s = math.cos(theta), math.sin(theta)
    fx, fy = rho * c, rho * s
    half = masks.half_width(4.71)
    seg = MR.segment(0, fx - 100.0 * -s, fy - 100.0 * c, fx + 100.0 * -s, fy + 100.0 * c, half=half, cap=np.inf)
    mask, stats, _ = MR.mask_trails([seg], (1, *shape))
    held = flux[mask[0] != 0].sum() / flux.sum()
    bound = MR.band_flux_fraction(half)
    assert bound == math.erf((half - 1.0) / (2.0 * math.sqrt(2.0))) and 0.99 < bound < 1.0
    print("held %.6f, bound %.6f" % (held, bound))
    assert held >= bound
    assert int(stats[0]["n_pix"]) == int((mask != 0).sum()) > 0


def test_pack_and_unpack():
    rng = np.random.default_rng(2)
    for shape in ((3, 37, 130), (1, 1, 1), (17, 65)):
        m = (rng.random(shape) < 0.3).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
        bits, shp = masks.pack(m)
        assert shp == shape and bits.dtype == np.uint8
        n = 1 if len(shape) == 2 else shape[0]
        assert bits.shape == (n, (shape[-2] * shape[-1] + 7) // 8)
        back = masks.unpack(bits, shp)
        assert back.shape == shape and back.dtype == np.uint8 and np.array_equal(back, (m != 0).astype(np.uint8))
    with pytest.raises(ValueError):
        masks.pack(np.zeros(5, np.uint8))


def test_segment_builders():
    tr = np.zeros(4, _native.TRAIL_DTYPE)
    tr["status"] = [_native.TRAIL_OK, _native.TRAIL_NOT_FOUND, _native.TRAIL_OK, _native.TRAIL_TOO_FAINT]
    for k, v in (("x1", 1.5), ("y1", 2.5), ("x2", 300.25), ("y2", 40.0)):
        tr[k] = v
    tr["x1"][2] = 9.0
    tr["fwhm"] = [4.71, np.nan, np.nan, 5.0]
    segs, keep = masks.segments_from_trails(tr, bits=2, cap=3.0, fill=1.25)
    assert keep == [0, 2] and segs.dtype == masks.SEGMENT_DTYPE
    assert segs["frame"].tolist() == [0, 2] and segs["bits"].tolist() == [2, 2] and segs["cap"].tolist() == [3.0, 3.0]
    assert segs["half"].tolist() == [6.71, 10.0] and segs["fill"].tolist() == [1.25, 1.25]
    assert [tuple(s[k] for k in ("x1", "y1", "x2", "y2")) for s in segs] == [(1.5, 2.5, 300.25, 40.0), (9.0, 2.5, 300.25, 40.0)]
    segs, keep = masks.segments_from_trails(tr, frames=[7, 8, 9, 10], grow=0.0)
    assert segs["frame"].tolist() == [7, 9] and segs["half"].tolist() == [4.71, 8.0]
    with pytest.raises(TypeError):
        masks.segments_from_trails(tr, no_such=1)

    st = np.zeros(3, _native.STACK_DTYPE)
    st["status"] = [_native.STACK_OK, _native.STACK_TOO_SHORT, _native.STACK_TOO_FAINT]
    st["x2"], st["y2"], st["fwhm"] = 50.0, 60.0, 8.0
    sg = np.zeros(3, _native.STACK_SEGMENT_DTYPE)
    sg["frame"] = [4, 5, 6]
    segs, keep = masks.segments_from_stack(st, sg)
    assert keep == [0] and segs["frame"].tolist() == [4] and segs["half"].tolist() == [10.0] and segs["x2"].tolist() == [50.0]
    with pytest.raises(ValueError):
        masks.segments_from_stack(st, sg[:2])

    lines = np.zeros((3, 2), _native.RADON_LINE_DTYPE)
    lines["ex1"], lines["ey1"], lines["ex2"], lines["ey2"] = 1.0, 2.0, 3.0, 4.0
    lines["ex2"][2, 1] = 33.0
    segs, where = masks.segments_from_radon_lines(lines, [1, 0, 2])
    assert where == [(0, 0), (2, 0), (2, 1)] and segs["frame"].tolist() == [0, 2, 2]
    assert segs["half"].tolist() == [10.0] * 3 and segs["x2"].tolist() == [3.0, 3.0, 33.0] and segs["y1"].tolist() == [2.0] * 3
    segs, _ = masks.segments_from_radon_lines(lines, [1, 0, 2], fwhm=[6.0, np.nan, 1.0])
    assert segs["half"].tolist() == [8.0, 10.0, 6.0]

    rows = [{"x1": -900, "y1": 50, "x2": 1100, "y2": 60}, {"x1": 0, "y1": -1000, "x2": 10, "y2": 1000}]
    segs = masks.segments_from_results(rows, fwhm=[np.nan, 4.71], bits=8)
    assert segs["frame"].tolist() == [0, 1] and segs["half"].tolist() == [10.0, 6.71] and segs["bits"].tolist() == [8, 8]
    assert segs["x1"].tolist() == [-900.0, 0.0] and segs["y2"].tolist() == [60.0, 1000.0]
    assert masks.segments_from_results(rows, frames=[3, 3])["frame"].tolist() == [3, 3]
    # end points far off the image are what the definition allows: the band crosses the whole frame
    mask, stats, _ = MR.mask_trails(masks.segments_from_results(rows[:1]), (1, 100, 200))
    assert tuple(stats[0])[0] == MR.OK and mask[0].any(axis=0).all()


def test_masks_row_format(tmp_path):
    seg = masks.segments([(0, 1.5, 2.25, 300.125, 0.1, 6.71)])[0]
    row = masks.format_row((94, 1, "r", 100), "detect", 0, seg, 1234)
    assert row == "94 1 r 100 detect 0 1.5 2.25 300.125 0.1 6.71 1234"
    assert len(row.split()) == len(masks.MASK_COLUMNS)
    p = tmp_path / "masks.txt"
    p.write_text(row + "\n" + masks.format_row((94, 1, "r", 101), "radon", 2, seg, 0) + "\n")
    back = masks.read_masks(str(p))
    assert back[0] == dict(zip(masks.MASK_COLUMNS, (94, 1, "r", 100, "detect", 0, 1.5, 2.25, 300.125, 0.1, 6.71, 1234)))
    assert back[1]["source"] == "radon" and back[1]["line"] == 2 and back[1]["n_pix"] == 0
