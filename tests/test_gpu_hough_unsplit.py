"""Whole pixel lists on narrow angle slabs (run_hough's shape for large batches), forced on single small frames with
LFDMI_VOTE_AW: slabs of 64, 32, 16 and 8 angles, partial last slabs, guard bins, empty and very short and long lists, and the
whole pipe with the narrow shape forced and off.  Frames are built the way tests/hough_cases.py builds them; every
comparison is exact against the oracle's accumulator (guard cells included) and line list.

A batch takes the narrow shape by itself once 23 slabs x images x frames reach LFDMI_VOTE_WGS workgroups; with LFDMI_VOTE_WGS=1
that is every launch, which test_gpu_hough_shapes.py::test_process_wide_knobs_in_a_fresh_process runs (the knob is read once
per process).

Not reachable through the library's entry points, so not here: a two-image launch whose box image is empty (a pass reaches
HoughLines only after a rectangle was drawn into it); the 90 : 1 lists of hough_cases.p_noise_streak stand in for it."""
import math

import numpy as np
import pytest

import hough_cases as H

pytestmark = pytest.mark.gpu

H_, W_ = 96, 160
WIDTHS = (6, 5, 4, 3)          # LFDMI_VOTE_AW; 6 is the width that fits these frames: the pieces, as without the knob
_REF = {}


def forced_chunks(h, w, rho, theta, awl, classes=True):
    """(cm_a, cm_b) of run_hough when slabs of 1 << awl angles are forced: hough_cases.vote_shape's rule at that width"""
    na, _ = H.hough_dims(h, w, rho, theta)
    cos, _ = H.trig_table(na, rho, theta)
    AW = 1 << awl
    lmax = []
    for sl in range(-(-na // AW)):
        cmax = float(np.abs(cos[sl * AW:(sl + 1) * AW]).astype(np.float64).max())
        lmax.append(int(min(H.CHUNK_MAX, max(1, math.floor(0.999 / cmax) + 1 if cmax > 0 else H.CHUNK_MAX))))
    cm_a = min(lmax)
    b = [l for l in lmax if l >= 2 * cm_a]
    return cm_a, (min(b) if b and classes else 0)


def few(h, w, n=5):
    """n short runs: fewer chunks than a workgroup has waves"""
    a = np.zeros((h, w), np.uint8)
    for k in range(n):
        a[7 + 13 * k, 11 + 17 * k:11 + 17 * k + 3 + k] = 255
    return a


def one(h, w):
    a = np.zeros((h, w), np.uint8)
    a[h // 3, w - 2] = 9
    return a


FRAMES = dict(H.FRAMES, few=few, one=one)


def ref(oracle, frame, h, w, rho, div):
    """(image, oracle accumulator, {threshold: (lines, n)}) at thresholds 1 and half the maximum, once, read-only"""
    key = (frame, h, w, rho, div)
    if key not in _REF:
        img = FRAMES[frame](h, w)
        theta = math.pi / div
        acc = oracle.hough_accum(img, rho, theta)
        lines = {thr: oracle.hough_lines(img, rho, theta, threshold=thr) for thr in (1, max(2, int(acc.max()) // 2))}
        img.setflags(write=False)
        acc.setflags(write=False)
        _REF[key] = (img, acc, lines)
    return _REF[key]


def check(oracle, monkeypatch, frame, h, w, rho, div, awl):
    from lfd_amd import _native
    img, acc_o, lines_o = ref(oracle, frame, h, w, rho, div)
    theta = math.pi / div
    monkeypatch.setenv("LFDMI_VOTE_AW", str(awl))
    with _native.Context(0, h, w, 1, caps="worst") as ctx:
        acc = ctx.hough_accum(img, rho, theta)
        cnt = ctx.get_counters(0, 1)[0]
        got = {thr: ctx.hough_lines(img, rho, theta, threshold=thr) for thr in lines_o}
        assert ctx.spill_count() == 0
    assert acc.shape == acc_o.shape
    assert np.array_equal(acc, acc_o), (np.argwhere(acc != acc_o)[:8], int((acc != acc_o).sum()))
    for thr, (l_o, n_o) in lines_o.items():
        l_g, n_g = got[thr]
        assert n_g == n_o and ((l_g is None and l_o is None) or np.array_equal(l_g, l_o)), (thr, n_g, n_o)
    return cnt


@pytest.mark.parametrize("awl", WIDTHS)
@pytest.mark.parametrize("rho", [20.0, 5.0])
@pytest.mark.parametrize("frame", ["rand", "runs"])
def test_forced_widths(oracle, monkeypatch, frame, rho, awl):
    """180 angles: the last slab has 52 angles at AW 64, 20 at AW 32, 4 at AW 16 and AW 8.  `rand` has more than 64 x 16 chunks (a
    wave takes several batches of 64).  The lists are cut for the forced width's slabs: list B's length shows the width taken."""
    cnt = check(oracle, monkeypatch, frame, H_, W_, rho, 180, awl)
    img = FRAMES[frame](H_, W_)
    cm_a, cm_b = forced_chunks(H_, W_, rho, math.pi / 180, awl)
    assert (cm_a, cm_b) == (int(rho), {20.0: {6: 0, 5: 46, 4: 46, 3: 42}, 5.0: {6: 0, 5: 12, 4: 12, 3: 11}}[rho][awl])
    n_a = len(H.chunk_list(img, cm_a)[0])
    assert frame != "rand" or n_a > 64 * 16
    assert cnt[H.C_OVERFLOW] == 0 and cnt[H.C_NNZ_EQU] == np.count_nonzero(img)
    assert cnt[H.C_NPIX_EQU] == n_a and cnt[H.C_NPIXB_EQU] == (len(H.chunk_list(img, cm_b)[0]) if cm_b else 0)


@pytest.mark.parametrize("awl", [4, 3])
@pytest.mark.parametrize("div", [176, 17, 9])
def test_other_numangle(oracle, monkeypatch, div, awl):
    """numangle a multiple of the slab width (176), and the width plus one (17 at AW 16, 9 at AW 8: a last slab of one angle)"""
    check(oracle, monkeypatch, "runs", H_, W_, 20.0, div, awl)


@pytest.mark.parametrize("awl", WIDTHS)
def test_guard_bins(oracle, monkeypatch, awl):
    """16 rows at rho 100 (hough_cases' r100_thin_full): x cos / rho alone rounds one bin past the last row, into OpenCV's guard cell"""
    check(oracle, monkeypatch, "full", 16, 4000, 100.0, 180, awl)
    _, acc_o, _ = ref(oracle, "full", 16, 4000, 100.0, 180)
    assert acc_o[:, 0].any() or acc_o[:, -1].any()


@pytest.mark.parametrize("awl", [6, 4, 3])
@pytest.mark.parametrize("frame", ["empty", "one", "few", "full"])
def test_odd_lists(oracle, monkeypatch, frame, awl):
    """no pixel, one pixel, five chunks (most waves have nothing to do), every pixel (full words: the longest chunks)"""
    check(oracle, monkeypatch, frame, H_, W_, 20.0, 180, awl)


def test_a_dirty_accumulator_between_widths(oracle, monkeypatch):
    """one context per width, frames of falling content: the store path leaves nothing of the frame before, the empty frame last"""
    from lfd_amd import _native
    for awl in (4, 3):
        monkeypatch.setenv("LFDMI_VOTE_AW", str(awl))
        with _native.Context(0, H_, W_, 1, caps="worst") as ctx:
            for frame in ("full", "rand", "few", "empty"):
                img, acc_o, _ = ref(oracle, frame, H_, W_, 20.0, 180)
                assert np.array_equal(ctx.hough_accum(img, 20.0), acc_o), (awl, frame)


@pytest.mark.parametrize("awl", [4, 3])
@pytest.mark.parametrize("name", ["noise_streak", "thin"])
def test_two_images(oracle, monkeypatch, name, awl):
    """process_bright (rho 20) and process_dim (rho 5) with whole lists: image 0's list 90 times image 1's, and both alike"""
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    pb, pd, _ = default_params()
    monkeypatch.setenv("LFDMI_VOTE_AW", str(awl))
    frame = H.PASS_FRAMES[name]()
    h, w = frame.shape
    with _native.Context(0, h, w, 1, caps="worst") as ctx:
        for which, rho in (("bright", 20.0), ("dim", 5.0)):
            p = dict(pd if which == "dim" else pb, houghMethod=rho)
            want, equ_o, box_o = (oracle.process_dim if which == "dim" else oracle.process_bright)(frame.copy(), p, want_images=True)
            res, le, lb = (ctx.process_dim if which == "dim" else ctx.process_bright)(frame.copy(), p)
            assert want["detection"] == 1 and all(res[k].item() == v for k, v in want.items()), (which, want, res)
            K = p["nlinesInSet"]
            for img, lg, n_g in ((equ_o, le, res["n_lines_equ"]), (box_o, lb, res["n_lines_box"])):
                l_o, n_o = oracle.hough_lines(img, rho, threshold=1, max_lines=K)
                k = min(K, n_o)
                assert n_g == n_o and (k == 0 or np.array_equal(lg[:k], l_o.reshape(-1, 2)[:k])) and not lg[k:].any(), which


def test_whole_pipe_narrow_and_off(oracle, monkeypatch):
    """detect_batch on 8 small synthetic frames with slabs of 8 angles forced and with the width that fits (the pieces): the
    records equal each other and the oracle's"""
    from lfd_amd import _native, synth
    from lfd_amd.detecttrails import default_params
    pb, pd, _ = default_params()
    frames = np.stack([synth.make_frame(k, shape=(256, 320), with_catalog=False)[0] for k in range(8)])
    want = [oracle.detect_frame(f.copy(), pb, pd) for f in frames]
    assert sum(r["detection"] for r in want) >= 2                            # HoughLines runs
    got = {}
    for awl in ("3", "6"):
        monkeypatch.setenv("LFDMI_VOTE_AW", awl)
        with _native.Context(0, 256, 320, 8) as ctx:
            got[awl] = ctx.detect_batch(frames.copy(), pb, pd)
    assert got["3"].dtype == got["6"].dtype and got["3"].tobytes() == got["6"].tobytes()
    for i in range(8):
        assert all(got["3"][i][k].item() == v for k, v in want[i].items()), (i, want[i], got["3"][i])
