"""``lfd_amd.recovery`` for short trails, without a GPU: ``shorten`` cuts every trail of a plan to a fraction of its crossing at
a random place and leaves the plan's own random stream alone; the new detector name and the command line's new flag."""
import numpy as np
import pytest


def test_shorten_keeps_the_plan_and_cuts_inside_the_crossing():
    from lfd_amd import recovery as RC
    shape = (372, 512)
    plan = RC.draw_trails(40, shape, 7, [0.02, 0.05])
    assert RC.shorten(plan, shape, 1.0, 7) is plan                                  # the default: today's plan
    cut = RC.shorten(plan, shape, 0.25, 7)
    assert RC.plan_checksum(plan) == RC.plan_checksum(RC.draw_trails(40, shape, 7, [0.02, 0.05]))   # (plan untouched)
    for k in ("frame", "peak", "rho", "theta"):
        assert np.array_equal(cut[k], plan[k]), k
    pos = []
    for a, b in zip(plan, cut):
        ta, tb = RC.extent(float(a["rho"]), float(a["theta"]), -np.inf, np.inf, shape)
        assert ta - 1e-9 <= b["t0"] < b["t1"] <= tb + 1e-9
        assert abs((b["t1"] - b["t0"]) - 0.25 * (tb - ta)) <= 1e-9 * (tb - ta)
        pos.append((b["t0"] - ta) / (0.75 * (tb - ta)))
    assert min(pos) < 0.2 and max(pos) > 0.8                                        # anywhere along the crossing
    again = RC.shorten(plan, shape, 0.25, 7)
    assert RC.plan_checksum(again) == RC.plan_checksum(cut) != RC.plan_checksum(RC.shorten(plan, shape, 0.25, 8))
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            RC.shorten(plan, shape, bad, 7)


def test_detector_names():
    from lfd_amd import recovery as RC
    with pytest.raises(ValueError) as e:
        RC.run(None, np.zeros((1, 8, 8), np.float32), None, None, None, None, 1.0, detector="radon-long")
    assert "radon-short" in str(e.value)
