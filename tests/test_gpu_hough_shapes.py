"""k_pixlist / k_hough_vote / k_hough_peaks off the default launch shape: every slab width (AW 32 .. 2), more than 32 slabs, the
direct-store flush, every list split, both chunk classes, sides of 8191 and other numangle -- the named cases of
tests/hough_cases.py (their shapes are checked on the CPU in tests/test_hough_cases_model.py) against the oracle's
accumulators and line lists.  Votes are integers: every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hough_cases as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def ref(oracle, name):
    """(frame, oracle accumulator) of a case, computed once and read-only"""
    if name not in _REF:
        c = H.BY_NAME[name]
        img = H.frame(c)
        acc = oracle.hough_accum(img, c["rho"], c["theta"])
        img.setflags(write=False)
        acc.setflags(write=False)
        _REF[name] = (img, acc)
    return _REF[name]


def context(case, monkeypatch, env, slots=1, caps="worst"):
    """a context sized to the case; the knobs stay set while it lives (the spill workspace reads them when it is created)"""
    from lfd_amd import _native
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, w = H.ctx_dims(case)
    return _native.Context(0, h, w, slots, caps=caps)


def same_lines(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


@pytest.mark.parametrize("variant", H.VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c["name"])
def test_accumulator(oracle, monkeypatch, case, variant):
    vid, env = variant
    img, acc_o = ref(oracle, case["name"])
    s = H.variant_shape(case, env)
    with context(case, monkeypatch, env) as ctx:
        acc = ctx.hough_accum(img, case["rho"], case["theta"])
        cnt = ctx.get_counters(0, 1)[0]
        assert ctx.spill_count() == 0
    assert acc.shape == acc_o.shape
    assert np.array_equal(acc, acc_o), (np.argwhere(acc != acc_o)[:8], int((acc != acc_o).sum()))
    # the lists the vote read: every pixel once in each, cut every cm_a / cm_b inside its 64-pixel word
    assert cnt[H.C_OVERFLOW] == 0 and cnt[H.C_NNZ_EQU] == np.count_nonzero(img)
    assert cnt[H.C_NPIX_EQU] == len(H.chunk_list(img, s["cm_a"])[0])
    assert cnt[H.C_NPIXB_EQU] == (len(H.chunk_list(img, s["cm_b"])[0]) if s["cm_b"] else 0)


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c["name"])
def test_lines(oracle, monkeypatch, case):
    """k_hough_peaks and the sort on the same accumulators: the full line list at threshold 1 and at a higher one (the count
    alone where the list has more than 10^5 lines)"""
    img, acc_o = ref(oracle, case["name"])
    rho, theta = case["rho"], case["theta"]
    thr_hi = max(2, int(acc_o.max()) // 2)
    with context(case, monkeypatch, {}) as ctx:
        for thr in (1, thr_hi):
            l_o, n_o = oracle.hough_lines(img, rho, theta, threshold=thr)
            if n_o < 100_000:
                l_g, n_g = ctx.hough_lines(img, rho, theta, threshold=thr)
                assert n_g == n_o and same_lines(l_g, l_o), (thr, n_g, n_o)
            else:
                l_g, n_g = ctx.hough_lines(img, rho, theta, threshold=thr, max_lines=64)
                assert n_g == n_o and np.array_equal(l_g, l_o[:64]), (thr, n_g, n_o)


@pytest.mark.parametrize("split", ["1", "4"])
def test_rho_below_the_default_capacity_goes_to_the_spill_workspace(oracle, monkeypatch, split):
    """default capacities hold accumulators down to rho = 5: rho = 1 runs in the worst-case workspace, created on first use
    with the same knobs"""
    case = H.BY_NAME["aw16_r1_rand"]
    img, acc_o = ref(oracle, case["name"])
    with context(case, monkeypatch, {"LFDMI_VOTE_SPLIT": split}, caps=None) as ctx:
        before = ctx.workspace_bytes()
        assert np.array_equal(ctx.hough_accum(img, case["rho"], case["theta"]), acc_o)
        assert ctx.workspace_bytes() > before                                     # the spill workspace exists now
        l_o, n_o = oracle.hough_lines(img, case["rho"], case["theta"], threshold=3)
        l_g, n_g = ctx.hough_lines(img, case["rho"], case["theta"], threshold=3)
        assert n_g == n_o and same_lines(l_g, l_o)


def test_direct_store_on_a_dirty_accumulator(oracle, monkeypatch):
    """LFDMI_VOTE_SPLIT=1: the slab is stored, not merged, and nothing clears the accumulator beforehand: after the all-255
    frame every later result, guard rows and columns included, must still be the oracle's"""
    big = H.BY_NAME["aw8_r1_full"]
    with context(big, monkeypatch, {"LFDMI_VOTE_SPLIT": "1"}) as ctx:
        assert H.variant_shape(big, {"LFDMI_VOTE_SPLIT": "1"})["nsplit"] == 1
        for name in ("aw8_r1_full", "aw8_r1_corner", "r20_class_b", "aw8_r1_full", "r100_thin_full", "aw16_r1_rand", "aw8_r1_empty"):
            c = H.BY_NAME[name]
            assert c["h"] <= big["h"] and c["w"] <= big["w"]                       # (r20_class_b: a smaller shape AND a coarser rho)
            img, acc_o = ref(oracle, name)
            acc = ctx.hough_accum(img, c["rho"], c["theta"])
            assert np.array_equal(acc, acc_o), name
            assert not acc[0].any() and not acc[-1].any()
            assert name == "r100_thin_full" or (not acc[:, 0].any() and not acc[:, -1].any())   # (that one votes into a guard bin)


@pytest.mark.parametrize("split", ["1", "4"])
def test_batch_through_two_slots(oracle, monkeypatch, split):
    """three frames of different content through a context of two slots (two chunks, slot 0 used twice): each equals its
    single-frame result"""
    case = H.BY_NAME["aw16_r5_runs"]
    frames = np.stack([H.FRAMES[f](case["h"], case["w"]) for f in ("full", "runs", "corner")])
    want = [oracle.hough_accum(f, case["rho"], case["theta"]) for f in frames]
    with context(case, monkeypatch, {"LFDMI_VOTE_SPLIT": split}, slots=2) as ctx:
        acc = ctx.hough_accum(frames, case["rho"], case["theta"])
        lines, n = ctx.hough_lines(frames, case["rho"], case["theta"], threshold=40)
        again = ctx.hough_accum(frames[::-1].copy(), case["rho"], case["theta"])
    for i in range(3):
        assert np.array_equal(acc[i], want[i]) and np.array_equal(again[2 - i], want[i]), i
        l_o, n_o = oracle.hough_lines(frames[i], case["rho"], case["theta"], threshold=40)
        assert n[i] == n_o and same_lines(lines[i], l_o), i


_PASS = {}


def pass_ref(oracle, name, which, rho):
    """oracle record and Hough input images of a two-image frame, once"""
    from lfd_amd.detecttrails import default_params
    key = (name, which, rho)
    if key not in _PASS:
        pb, pd, _ = default_params()
        p = dict(pd if which == "dim" else pb, houghMethod=rho)
        fn = oracle.process_dim if which == "dim" else oracle.process_bright
        _PASS[key] = (p,) + fn(H.PASS_FRAMES[name]().copy(), p, want_images=True)
    return _PASS[key]


def test_two_image_frames_are_what_they_are_named_for(oracle):
    n = {}
    for name in H.PASS_FRAMES:
        _, res, equ, box = pass_ref(oracle, name, "bright", 20.0)
        assert res["detection"] == 1 and pass_ref(oracle, name, "dim", 5.0)[1]["detection"] == 1   # both passes reach HoughLines
        n[name] = (len(H.chunk_list(equ, 20)[0]), len(H.chunk_list(box, 20)[0]))
    assert n["noise_streak"][0] > 50 * n["noise_streak"][1] > 0
    assert 0.8 < n["thin"][0] / n["thin"][1] < 1.25
    assert 0 < n["bar"][1] < 100


@pytest.mark.parametrize("split,balance", H.PASS_VARIANTS)
@pytest.mark.parametrize("name", sorted(H.PASS_FRAMES))
def test_two_images_share_the_pieces(oracle, monkeypatch, name, split, balance):
    """process_bright (rho 20) and process_dim (rho 5): HoughLines on the equalised and on the box image in one launch, the
    pieces of each slab shared out by list length (LFDMI_VOTE_BALANCE) or half and half"""
    from lfd_amd import _native
    monkeypatch.setenv("LFDMI_VOTE_SPLIT", split)
    monkeypatch.setenv("LFDMI_VOTE_BALANCE", balance)
    frame = H.PASS_FRAMES[name]()
    h, w = frame.shape
    s = H.vote_shape(h, w, 20.0, vote_split=int(split), n_img=2, balance=balance != "0")
    assert s["nsplit"] == int(split) and s["balance"] == int(balance)
    with _native.Context(0, h, w, 1, caps="worst") as ctx:
        for which, rho in (("bright", 20.0), ("dim", 5.0)):
            p, want, equ_o, box_o = pass_ref(oracle, name, which, rho)
            fn = ctx.process_dim if which == "dim" else ctx.process_bright
            res, le, lb = fn(frame.copy(), p)
            assert all(res[k].item() == v for k, v in want.items()), (which, want, res)
            assert want["detection"] == 1
            K = p["nlinesInSet"]
            for stage, lg, n_g in ((_native.STAGE_EQU, le, res["n_lines_equ"]), (_native.STAGE_BOX, lb, res["n_lines_box"])):
                img = ctx.get_stage(0, stage, h, w)
                assert np.array_equal(img != 0, (equ_o if stage == _native.STAGE_EQU else box_o) != 0)
                l_o, n_o = oracle.hough_lines(img, rho, threshold=1, max_lines=K)
                assert n_g == n_o, (which, stage)
                k = min(K, n_o)
                assert k == 0 or np.array_equal(lg[:k], l_o.reshape(-1, 2)[:k]), (which, stage)
                assert not lg[k:].any()


def test_side_of_8192_is_refused():
    """y and x0 have 13 bits each in a list entry: a side of 8192 is an argument error, not a wrapped coordinate"""
    from lfd_amd import _native
    for h, w in ((16, 8192), (8192, 16)):
        with pytest.raises(_native.NativeError) as e:
            _native.Context(0, h, w, 1)
        assert e.value.code == _native.ERR_ARG
    with _native.Context(0, 16, 8191, 1, caps="worst") as ctx:
        for shape in ((16, 8192), (17, 8191)):
            with pytest.raises(_native.NativeError) as e:
                ctx.hough_accum(np.zeros(shape, np.uint8), 1.0)
            assert e.value.code == _native.ERR_CAPACITY
        assert not ctx.hough_accum(np.zeros((16, 8191), np.uint8), 1.0).any()


def test_process_wide_knobs_in_a_fresh_process(oracle, tmp_path):
    """LFDMI_VOTE_THREADS=64 (one wave per workgroup), LFDMI_VOTE_WGS=1 (lists never split: the store path) and
    LFDMI_PEAK_ROWS=8 are read once per process: one child interpreter runs five cases against the oracle's results"""
    names = ("aw32_r5_runs", "aw2_r1_runs", "t_aw32_r4_walk", "th2048_32slabs", "r100_thin")
    data = {}
    for name in names:
        c = H.BY_NAME[name]
        img, acc_o = ref(oracle, name)
        l_o, n_o = oracle.hough_lines(img, c["rho"], c["theta"], threshold=1)
        data["acc_" + name], data["lines_" + name], data["n_" + name] = acc_o, l_o, np.int64(n_o)
    npz = tmp_path / "hough_ref.npz"
    np.savez(npz, **data)
    env = dict(os.environ, LFDMI_VOTE_THREADS="64", LFDMI_VOTE_WGS="1", LFDMI_PEAK_ROWS="8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_hough_child.py"), str(npz)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert [line.split()[0] for line in r.stdout.splitlines() if line.endswith(" ok")] == sorted(names)
