"""DetectTrails(trail_masks=True) end to end on the synthetic tree of tests/test_gpu_dropin.py: masks.txt has one row per
results.txt row, in order, whose pixel count is the restatement's (tests/mask_ref.py); the .npz planes unpack to the
restatement's masks; results.txt and profiles.txt do not change with the option; rank files concatenate to the one-process file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as MR  # noqa: E402
import test_gpu_dropin as TD  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (512, 768)
FIELDS = list(range(0, 7))


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("batch", [1, 4])
def test_masks_rows_and_planes_equal_the_restatement(tmp_path, batch):
    from lfd_amd import masks
    from lfd_amd.detecttrails import DetectTrails
    TD.build_tree(tmp_path, FIELDS, SHAPE)
    plain, masked, mdir = tmp_path / "plain", tmp_path / "masked", tmp_path / "planes"
    plain.mkdir()
    masked.mkdir()
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(plain), trail_profiles=True).process(batch=batch)
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(masked), trail_profiles=True, trail_masks=True, mask_dir=str(mdir))
    assert dt.masks_file == str(masked / "masks.txt")
    dt.process(batch=batch)
    # every other output is byte for byte what it is without the option
    for name in ("results.txt", "profiles.txt", "errors.txt"):
        assert read(masked / name) == read(plain / name), name
    res = [ln.split() for ln in open(dt.results) if ln.strip()]
    prof = [ln.split() for ln in open(dt.profiles) if ln.strip()]
    rows = masks.read_masks(dt.masks_file)
    assert len(res) >= 2 and len(rows) == len(res) == len(prof)
    assert [[str(r[k]) for k in ("run", "camcol", "filter", "field")] for r in rows] == [r[:4] for r in res]     # the same order
    measured = 0
    for r, p in zip(rows, prof):
        assert r["source"] == "detect" and r["line"] == 0
        fwhm = float(p[4 + 13])                                                   # profiles.txt: the key, then TRAIL_DTYPE's fields
        assert r["half"] == masks.half_width(fwhm)
        if int(p[4]) == 0:                                                        # a measured trail: its refined extent
            measured += 1
            assert [r[k] for k in ("x1", "y1", "x2", "y2")] == [float(v) for v in p[4 + 6:4 + 10]]
        seg = MR.segment(0, r["x1"], r["y1"], r["x2"], r["y2"], half=r["half"], cap=0.0)
        want, stats, _ = MR.mask_trails([seg], (1, *SHAPE))
        assert r["n_pix"] == int(stats[0]["n_pix"]) > 0
        with np.load(mdir / ("mask-%d-%d-%s-%d.npz" % (r["run"], r["camcol"], r["filter"], r["field"]))) as z:
            assert tuple(z["shape"]) == SHAPE
            assert np.array_equal(masks.unpack(z["bits"], z["shape"]), want[0])
    assert measured >= 1
    assert len(os.listdir(mdir)) == len(rows)                                     # a frame without a row has no plane


def test_rank_files_and_default_off(tmp_path):
    from lfd_amd.detecttrails import DetectTrails
    TD.build_tree(tmp_path, FIELDS, SHAPE)
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(one), trail_masks=True).process(batch=4)
    for r in (0, 1):
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(two), trail_masks=True).process(batch=2, rank=r, world_size=2)
    whole = read(one / "masks.txt")
    assert whole and read(two / "masks.txt.rank0") + read(two / "masks.txt.rank1") == whole
    # without trail_profiles: the results row's line and the default half-width
    from lfd_amd import masks
    rows = masks.read_masks(str(one / "masks.txt"))
    res = [ln.split() for ln in open(one / "results.txt") if ln.strip()]
    assert [[r[k] for k in ("x1", "y1", "x2", "y2")] for r in rows] == [[float(v) for v in x[-4:]] for x in res]
    assert all(r["half"] == masks.half_width(float("nan")) == 10.0 for r in rows)
    # the option is off by default, and a bad mask parameter is refused at construction
    off = tmp_path / "off"
    off.mkdir()
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(off)).process(batch=4)
    assert not os.path.exists(off / "masks.txt") and read(off / "results.txt") == read(one / "results.txt")
    with pytest.raises(TypeError):
        DetectTrails(run=94, camcol=1, filter="r", savepath=str(off), trail_masks=True, mask_params={"no_such": 1})


def test_found_faint_lines_get_radon_rows(tmp_path):
    """the three-frame tree of test_gpu_radon_lines: field 101 carries two faint trails and no detection, field 102 a bright one"""
    import math
    import inject_ref as IR
    from lfd_amd import inject as I, masks, radon, stack, synth
    from lfd_amd.detecttrails import DetectTrails
    rng = np.random.default_rng(11)
    frames = rng.normal(0, 0.025, (3, *SHAPE)).astype(np.float32)
    tr = np.zeros(3, IR.TRAIL_DTYPE)
    th, th2 = math.radians(115.0), math.radians(30.0)
    rho = 384 * math.cos(th) + 256 * math.sin(th)
    tr[0] = (1, 0, rho, th, -np.inf, np.inf, 0.02)
    tr[1] = (2, 0, rho, th, -np.inf, np.inf, synth.BRIGHT_PEAK)
    tr[2] = (1, 0, 400 * math.cos(th2) + 240 * math.sin(th2), th2, -np.inf, np.inf, 0.018)
    table, step = I.gaussian_table(2.0)
    IR.inject(frames, tr, I.normalise_peak(table).astype(np.float32), step)
    cats = [synth.make_portable_frame(k, SHAPE)[1] for k in range(3)]
    synth.write_boss_tree(tmp_path, list(frames), cats, field0=100, filter="r")
    kw = {"radon": True, "radon_lines": 3, "radon_profiles": True}
    plain, masked = tmp_path / "plain", tmp_path / "masked"
    plain.mkdir()
    masked.mkdir()
    DetectTrails(run=94, camcol=1, filter="r", savepath=str(plain), **kw).process(batch=4)
    dt = DetectTrails(run=94, camcol=1, filter="r", savepath=str(masked), trail_masks=True, mask_dir=str(masked / "planes"), **kw)
    dt.process(batch=4)
    for name in ("results.txt", "errors.txt", "radon.txt", "radon_segments.txt", "radon_profiles.txt"):
        assert read(masked / name) == read(plain / name), name
    rows = masks.read_masks(dt.masks_file)
    segs = radon.read_segments(dt.radon_segments_file)
    prof = stack.read_profiles(dt.radon_profiles_file)
    res = [ln.split() for ln in open(dt.results) if ln.strip()]
    assert [(r["field"], r["source"], r["line"]) for r in rows] == [(101, "radon", 0), (101, "radon", 1)] + [(int(x[3]), "detect", 0) for x in res]
    assert [x[3] for x in res] == ["102"] and len(segs) == 2 == len(prof)
    plane = np.zeros(SHAPE, np.uint8)
    for r, s, p in zip(rows, segs, prof):
        assert [r[k] for k in ("x1", "y1", "x2", "y2")] == [s[k] for k in ("ex1", "ey1", "ex2", "ey2")]
        assert r["half"] == masks.half_width(p["fwhm"] if p["status"] == stack.OK else float("nan"))
        want, stats, _ = MR.mask_trails([MR.segment(0, r["x1"], r["y1"], r["x2"], r["y2"], half=r["half"])], (1, *SHAPE))
        assert r["n_pix"] == int(stats[0]["n_pix"]) > 0
        plane |= want[0]
    with np.load(masked / "planes" / "mask-94-1-r-101.npz") as z:                 # one plane per frame: both lines
        assert np.array_equal(masks.unpack(z["bits"], z["shape"]), plane)
