"""Detection with the found catalogue against detection with the truth catalogue, on the CPU: the whole pipe of the oracle
(remove_stars -> flip -> bright -> dim) on ``synth.make_frame(k, shape=(372, 512))``, k = 0 .. 15, once with the frame's own
catalogue and once with ``lfd_amd.stars.to_catalog(stars_ref.find_stars(frame))``.

Measured: 14 of the 16 seeds give the same ``found`` class and the same (rho, theta) to the bit; the two left out are listed
below with what happens in them."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stars_ref as R  # noqa: E402

SHAPE = (372, 512)
SEEDS = range(16)
# seeds whose ``found`` class is not compared, each with its reason (at most 4)
LEFT_OUT = {
    4: "bright streak: the found catalogue blots 58 of the ridge's 1185 pixels, the truth catalogue 158; on the less blotted "
       "frame the bright pass's two line sets (243 / 211 lines against 293 / 215) differ by more than thetaTresh and check_theta "
       "rejects, and the dim pass finds nothing either: found 0 against 1",
    10: "bright streak: check_theta rejects the bright pass in the same way (229 / 164 lines against 328 / 106); the dim pass then "
        "finds the very line the truth run's bright pass reports: found 2 against 1, equal rho and theta (asserted below)",
}


@functools.lru_cache(maxsize=None)
def runs(k):
    from lfd_amd import synth
    from lfd_amd.detecttrails import default_params
    from oracle import lfd_oracle as O
    O.build()
    pb, pd, prs = default_params()
    rs = O.rs_params("r", **{key: v for key, v in prs.items() if key != "debug"})
    img, cat, truth = synth.make_frame(k, shape=SHAPE)
    rec, frec = R.find_stars(img)
    from lfd_amd import stars
    found_cat = R.frame_catalog(stars.to_catalog(rec[None], np.array([frec]), prs["pixscale"]), 0)     # the shipped step 8
    return truth, O.detect_frame(img.copy(), pb, pd, cat, rs), O.detect_frame(img.copy(), pb, pd, found_cat, rs), pb["houghMethod"]


def test_same_class_and_line():
    assert len(LEFT_OUT) <= 4
    n_found = 0
    for k in SEEDS:
        truth, a, b, rho_step = runs(k)
        print(k, truth["streak"], "truth catalogue", a["found"], a["rho"], a["theta"], "found catalogue", b["found"], b["rho"], b["theta"])
        assert a["status"] == 0 and b["status"] == 0
        if k not in LEFT_OUT:
            assert a["found"] == b["found"], k
        if a["found"] and b["found"]:
            n_found += 1
            assert abs(a["rho"] - b["rho"]) <= rho_step and abs(a["theta"] - b["theta"]) <= math.radians(1.0) * (1 + 1e-6), k
    assert n_found >= 5


def test_no_more_false_detections():
    false_truth = false_found = frames = 0
    for k in SEEDS:
        truth, a, b, _ = runs(k)
        if truth["streak"] == "none":
            frames += 1
            false_truth += bool(a["found"])
            false_found += bool(b["found"])
    print("no-streak frames", frames, "false detections: truth catalogue", false_truth, "found catalogue", false_found)
    assert frames >= 4 and false_found <= false_truth
