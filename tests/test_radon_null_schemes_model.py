"""The null schemes and the peel rounds on the CPU, on the restatement alone (tests/radon_null_schemes_ref.py), on the frames of
test_radon_null_model.py (372 x 512 crops, K = 16, bin 2, frame f's seed f): where a noise frame's own peak lies among its nulls
under each scheme, how far a sigma-2 trail of peak 0.02 moves its frame's null range (the scramble: 0.13 - 0.46), what the row
shift makes of a trail along the rows, and round 1's null range against round 0's on a frame with two trails.

Every figure below was measured on all sixteen frames; to keep the test quick it runs eight of them, every second one (two per
orientation), whose extremes cannot exceed the sixteen's.  A bound is the sixteen frames' measured extreme times 1.5 for another
seed, the rule of test_radon_lines_model.PART_TOL and of test_sub_model.py."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import radon_lines_ref as L  # noqa: E402
import radon_null_schemes_ref as NS  # noqa: E402
import radon_ref as R  # noqa: E402
import test_radon_model as TM  # noqa: E402

K = 16
USED = list(range(0, TM.SET_SIZE, 2))      # eight of the sixteen frames: orientations 0, 0, 1, 1, 2, 2, 3, 3
OUTSIDE_AT_MOST = 2                         # a condition, as in test_radon_null_model.py.  Measured over sixteen frames: signflip 0,
#                                             rowshift 1 (frame 3, above its range), colshift 0; the scramble 1 (frame 3)
# How far the trail moves the largest / smallest null peak, measured over the sixteen frames (the scramble: +0.130 .. +0.452 and
# +0.178 .. +0.464):
#   signflip  -0.129 .. +0.176 and -0.072 .. +0.224: no mean is left in the null, what remains is the trail's variance
#   rowshift  largest peak, trails of q = 2, 3 (its own): +0.128 .. +0.518;  of q = 0, 1 (not its own): +0.086 .. +1.599
#   colshift  largest peak, trails of q = 0, 1 (its own): +0.138 .. +0.416;  of q = 2, 3 (not its own): +0.415 .. +2.506
# A shift keeps the mean as the scramble does, and the pieces of a trail that runs nearly along the shifted axis stay long.
SIGNFLIP_SHIFT, ROWSHIFT_OWN, COLSHIFT_OWN = 0.224, 0.518, 0.416
MARGIN = 1.5


def false_alarm(snr, null):
    from lfd_amd import radon
    return radon.false_alarm(snr, null)


@functools.lru_cache(maxsize=None)
def null_of(which, scheme):
    frames = (TM.noise_frames() if which == "noise" else TM.trail_frames())[USED]
    return NS.null_snr(frames, K, "lines", TM.SET_SIGMA, seeds=USED, scheme=scheme, bin=2)


def test_noise_placement_and_trail_shift_per_scheme():
    from lfd_amd import radon
    peak = np.array([TM.set_records("noise", 2)[f]["snr"] for f in USED], np.float32)
    trail = [TM.set_records("trail", 2)[f] for f in USED]
    own = {"rowshift": [f for f, g in enumerate(USED) if TM.SET_Q[g] >= 2], "colshift": [f for f, g in enumerate(USED) if TM.SET_Q[g] < 2]}
    assert all(radon.shift_scheme_for(TM.SET_Q[USED[f]]) == s for s, fs in own.items() for f in fs)
    for scheme in ("signflip", "rowshift", "colshift"):
        noise, with_trail = null_of("noise", scheme), null_of("trail", scheme)
        outside = (peak < noise.min(axis=1)) | (peak > noise.max(axis=1))
        up, lo = with_trail.max(axis=1) - noise.max(axis=1), with_trail.min(axis=1) - noise.min(axis=1)
        print(scheme, "noise nulls %.3f .. %.3f" % (noise.min(), noise.max()), "outside", [USED[f] for f in np.flatnonzero(outside)],
              "null max moves by", ["%.3f" % v for v in up], "null min by", ["%.3f" % v for v in lo])
        assert int(outside.sum()) <= OUTSIDE_AT_MOST
        assert 3.5 < float(noise.min()) and float(noise.max()) < 6.0               # the crops' ceiling, as under the scramble
        if scheme == "signflip":
            assert float(np.abs(up).max()) <= MARGIN * SIGNFLIP_SHIFT and float(np.abs(lo).max()) <= MARGIN * SIGNFLIP_SHIFT
        else:
            bound = MARGIN * (ROWSHIFT_OWN if scheme == "rowshift" else COLSHIFT_OWN)
            assert float(np.abs(up[own[scheme]]).max()) <= bound
        # derivable: no null reaches a found trail's score (17 - 25 against nulls below 8), so its estimate is 1 / (K + 1)
        assert float(with_trail.max()) < 8.0 < min(float(r["snr"]) for r in trail)
        assert all(false_alarm(r["snr"], n) == 1 / (K + 1) for r, n in zip(trail, with_trail))


def one_trail(deg):
    """noise frame 0 with a sigma-2 trail of peak 0.02 through its middle, the normal at ``deg`` degrees"""
    from lfd_amd import inject as I
    h, w = TM.SET_SHAPE
    th = math.radians(deg)
    tr = np.zeros(1, IR.TRAIL_DTYPE)
    tr[0] = (0, 0, (w / 2) * math.cos(th) + (h / 2) * math.sin(th), th, -np.inf, np.inf, TM.SET_PEAK)
    table, step = I.gaussian_table(2.0)
    return IR.inject(TM.noise_frames()[:1].copy(), tr, I.normalise_peak(table).astype(np.float32), step)


def test_rowshift_leaves_a_trail_along_the_rows_whole():
    """a trail exactly along the rows is the same in every column, so rotating its rows changes nothing: every row-shift null
    is the trail itself (measured: 25.04 .. 25.04 against the trail's 25.04) and its estimate is 1 up to the sums' last bits,
    while the column shift takes it apart (4.42 .. 5.45, estimate 1/17).  A trail at 45 degrees (score 20.70) is destroyed by both: 4.40 .. 5.19 and
    4.49 .. 5.75."""
    rows, diag = one_trail(90.0), one_trail(45.0)
    for name, f, whole in (("rows", rows, "rowshift"), ("diag", diag, None)):
        rec = R.search(f[0], TM.SET_SIGMA, bin=2)
        for scheme in ("rowshift", "colshift"):
            null = NS.null_snr(f, K, "lines", TM.SET_SIGMA, scheme=scheme, bin=2)[0]
            print(name, scheme, "null %.3f .. %.3f" % (null.min(), null.max()), "trail %.3f" % rec["snr"])
            if scheme == whole:
                # (the same pixels summed from another start: the float32 sums differ in their last bits only)
                assert float(np.abs(null - rec["snr"]).max()) <= 1e-5 * float(rec["snr"]) and float(null.min()) > 8.0
                assert false_alarm(rec["snr"] * np.float32(1 - 1e-5), null) == 1.0
            else:
                assert float(null.max()) < MARGIN * 5.75 < float(rec["snr"]) and false_alarm(rec["snr"], null) == 1 / (K + 1)


def test_round_one_is_held_against_a_frame_without_the_first_trail():
    """noise frame 1 with trails of peak 0.02 and 0.015 (scores 23.5 and 15.3; round 2 stops at 4.51).  Measured null ranges:
    round 0 4.088 .. 4.964, round 1 4.194 .. 5.190, round 2 4.134 .. 5.175; the frame without trails 4.151 .. 5.103.  The
    largest moves by 0.226 between rounds 0 and 1 and the smallest by 0.106; the bound is 1.5 times the larger."""
    from lfd_amd import inject as I
    h, w = TM.SET_SHAPE
    tr = np.zeros(2, IR.TRAIL_DTYPE)
    for i, (deg, pk) in enumerate(((110.0, 0.02), (60.0, 0.015))):
        th = math.radians(deg)
        tr[i] = (0, 0, (w / 2 + 20 * i) * math.cos(th) + (h / 2 - 30 * i) * math.sin(th), th, -np.inf, np.inf, pk)
    table, step = I.gaussian_table(2.0)
    f = IR.inject(TM.noise_frames()[1:2].copy(), tr, I.normalise_peak(table).astype(np.float32), step)
    recs, nl = L.search_lines(f[0], TM.SET_SIGMA, max_lines=3, bin=2)
    assert nl == 2
    rounds = NS.null_rounds(f, [recs], [nl], K, "lines", TM.SET_SIGMA, bin=2)[0]
    print("scores", ["%.2f" % r["snr"] for r in recs], "rounds", [("%.3f" % r.min(), "%.3f" % r.max()) for r in rounds])
    assert rounds.shape == (3, K) and not np.isnan(rounds).any()                   # rounds 0, 1 and the one that stopped the frame
    for k in (1, 2):
        assert abs(float(rounds[k].max() - rounds[0].max())) <= MARGIN * 0.226 and abs(float(rounds[k].min() - rounds[0].min())) <= MARGIN * 0.226
    assert all(false_alarm(recs[k]["snr"], rounds[k]) == 1 / (K + 1) for k in range(nl))
    assert false_alarm(recs[2]["snr"], rounds[2]) > 1 / (K + 1)                    # the round that stopped the frame lies among its nulls
