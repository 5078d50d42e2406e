"""The null peaks on the CPU, on the restatement alone (tests/radon_null_ref.py): that a frame's null peaks are its noise
ceiling -- the unscrambled peak of a noise frame lies among them -- and that a trail does not make its own ceiling: the null
peaks of a frame with a trail stay near those of the same frame without it, and the found line's false-alarm estimate is the
smallest K nulls can give.  The frames are those of test_radon_model.py, test_radon_short_model.py and test_radon_wide_model.py
at bin 2 with K = 16 and frame f's seed f."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_null_ref as NR  # noqa: E402
import radon_short_ref as S  # noqa: E402
import radon_wide_ref as W  # noqa: E402
import test_radon_model as TM  # noqa: E402
import test_radon_short_model as TS  # noqa: E402
import test_radon_wide_model as TW  # noqa: E402

K = 16                      # holds the condition below: 1 of the 16 noise frames peaks outside its null range (frame 3, above it)
OUTSIDE_AT_MOST = 2         # of 16: a condition, not a measurement
# How far a trail moves the ends of its frame's null range.  Scrambling keeps the frame's mean, and the trail's flux is in it:
# mean mu on every pixel adds mu sqrt(N) / sigma to every line of N pixels.  The sigma-2, peak-0.02 trails of test_radon_model.py
# hold 0.02 * 2 sqrt(2 pi) * ~550 px = 55 over 190464 pixels, mu = 2.9e-4, which is +0.5 on a line of 2000 pixels (the variance
# they add is 0.7 per cent).  Measured on the restatement over the 16 frames: the largest null peak rises by 0.13 .. 0.452, the
# smallest by 0.178 .. 0.464 -- against trail scores of 17.4 .. 24.9.  The bound is the measured extreme times 1.5 for another
# seed, the rule of test_radon_lines_model.PART_TOL.
LINES_SHIFT = 0.464
LINES_BOUND = 1.5 * LINES_SHIFT
# the same for the first quarter-length trail of test_radon_short_model.py (a quarter of the flux: +0.009 / +0.060) and the
# first sigma-6, peak-0.0045 trail of test_radon_wide_model.py (+0.383 / +0.459; scores 12.2 and 14.3)
SHORT_SHIFT, WIDE_SHIFT = 0.060, 0.459
SHORT_BOUND, WIDE_BOUND = 1.5 * SHORT_SHIFT, 1.5 * WIDE_SHIFT


def false_alarm(snr, null):
    from lfd_amd import radon
    return radon.false_alarm(snr, null)


@functools.lru_cache(maxsize=None)
def null_of(which):
    """float32 [16, K]: the lines' null peaks of test_radon_model's noise-only ('noise') or trail ('trail') frames, computed once"""
    frames = TM.noise_frames() if which == "noise" else TM.trail_frames()
    return NR.null_snr(frames, K, "lines", TM.SET_SIGMA, bin=2)


def test_a_noise_frames_own_peak_lies_among_its_null_peaks():
    null = null_of("noise")
    peak = np.array([r["snr"] for r in TM.set_records("noise", 2)], np.float32)
    outside = (peak < null.min(axis=1)) | (peak > null.max(axis=1))
    print("peak", ["%.2f" % v for v in peak], "null min", ["%.2f" % v for v in null.min(axis=1)], "null max",
          ["%.2f" % v for v in null.max(axis=1)], "outside", np.flatnonzero(outside).tolist())
    assert null.shape == (TM.SET_SIZE, K) and (null > 0).all()
    assert int(outside.sum()) <= OUTSIDE_AT_MOST
    # the frames' ceiling is the crops' (include/lfdmi.h step 5: 4.2 - 4.9 at bin 2, threshold 8), and no estimate is 0
    assert 3.5 < float(null.min()) and float(null.max()) < 6.0
    assert all(1 / (K + 1) <= false_alarm(p, n) <= 1.0 for p, n in zip(peak, null))


def test_a_trail_does_not_make_its_own_ceiling():
    noise, trail = null_of("noise"), null_of("trail")
    up, lo = trail.max(axis=1) - noise.max(axis=1), trail.min(axis=1) - noise.min(axis=1)
    print("null max moves by", ["%.3f" % v for v in up], "null min by", ["%.3f" % v for v in lo])
    assert float(np.abs(up).max()) <= LINES_BOUND and float(np.abs(lo).max()) <= LINES_BOUND
    recs = TM.set_records("trail", 2)
    assert all(r["found"] == 1 for r in recs)
    assert all(false_alarm(r["snr"], n) == 1 / (K + 1) for r, n in zip(recs, trail))          # exactly: no null reaches it
    assert float(trail.max()) < 8.0 < min(float(r["snr"]) for r in recs)


def one_kind(kind, noise_frame, trail_frame, search, bound):
    """one frame of a kind.  Its own peak among its K null peaks is asserted outright here, where the lines' sixteen frames
    may miss twice: with one frame and K = 16 exchangeable draws that holds with probability 15/17 for a seed not looked at,
    and it holds for these two frames (measured: 4.63 in 4.33 .. 5.12, 4.67 in 4.08 .. 5.08).  Whoever changes a seed here
    has to look again: a frame that falls outside is no fault of the code."""
    null = NR.null_snr(noise_frame[None], K, kind, TM.SET_SIGMA, bin=2)[0]
    with_trail = NR.null_snr(trail_frame[None], K, kind, TM.SET_SIGMA, bin=2)[0]
    peak = search(noise_frame, TM.SET_SIGMA, max_lines=1, bin=2)[0][0]["snr"]
    rec = search(trail_frame, TM.SET_SIGMA, max_lines=1, bin=2)[0][0]
    print(kind, "noise peak %.3f" % peak, "null %.3f .. %.3f" % (null.min(), null.max()), "with the trail %.3f .. %.3f" %
          (with_trail.min(), with_trail.max()), "trail %.2f" % rec["snr"])
    assert float(null.min()) <= float(peak) <= float(null.max())
    assert abs(float(with_trail.max() - null.max())) <= bound and abs(float(with_trail.min() - null.min())) <= bound
    assert rec["found"] == 1 and false_alarm(rec["snr"], with_trail) == 1 / (K + 1)


def test_short_kind_on_a_quarter_length_trail():
    noise = np.random.default_rng(TS.QUARTER_SEED).normal(0, TM.SET_SIGMA, (TM.SET_SIZE, *TS.QUARTER_SHAPE)).astype(np.float32)[0]
    one_kind("short", noise, TS.quarter_frames()[0], S.search_short, SHORT_BOUND)


def test_wide_kind_on_a_wide_faint_trail():
    one_kind("wide", TM.noise_frames()[0], TW.wide_trail_frames()[1][0], W.search_wide, WIDE_BOUND)
