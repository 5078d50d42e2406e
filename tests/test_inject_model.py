"""The host side of injection and recovery without a GPU: the tables against the defocus restatement, the numpy restatement of
the injection (tests/inject_ref.py) against answers derived by hand, the plan, the matching rule, the completeness table, the
text format, and the 16-frame recovery chain on the CPU (restatement + oracle) against its committed rows."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import defocus_ref as R  # noqa: E402
import inject_ref as IR  # noqa: E402

from lfd_amd import _native, inject, recovery, synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def physical_profile(g, h, fwhm):
    """O (x) D (x) S as tests/test_gpu_defocus.py builds it for its renderer"""
    o = np.ones(1) if not np.isfinite(h) else R.od(g, h, 0.0)
    return np.convolve(o, R.unit(R.seeing_raw(fwhm, g.delta)))


@pytest.mark.parametrize("h", [80.0, 100.0, 150.0, np.inf])
def test_defocus_table_equals_the_defocus_restatement(h):
    g = R.Grid()
    want = physical_profile(g, h, 1.43)
    got, step = inject.defocus_table(h, seeing_fwhm=1.43)
    assert got.shape == want.shape and len(got) % 2 == 1 and len(got) <= inject.MAX_TABLE
    assert step == g.step / g.ovs
    # The same expressions in double; only the order of a sum may differ.  A node is a sum of at most len(D) products of
    # values <= the factors' peaks, each normalisation a sum of at most n terms: reordering n non-negative terms moves a sum by
    # at most n eps relative, so a node moves by at most (n_D + n_S + n_conv) eps of the peak-sized partial sums.  With
    # n <= 2800 each that is below 3 * 2800 * 2^-53 = 1e-12 relative to the peak.
    n = len(want)
    assert n <= 2800
    assert np.abs(got - want).max() <= 3 * n * 2.0 ** -53 * want.max()
    assert abs(got.sum() - 1.0) <= 3 * n * 2.0 ** -53


def test_table_helpers():
    t, step = inject.gaussian_table(2.0, step=0.125)
    M = (len(t) - 1) // 2
    assert len(t) % 2 == 1 and t[M] == 1.0 and np.array_equal(t, t[::-1]) and M * step >= 12.0
    assert abs(inject.integral(t, step) - 2.0 * math.sqrt(2 * math.pi)) < 1e-6
    p = inject.normalise_peak(3.0 * t)
    assert p.max() == 1.0
    with pytest.raises(ValueError):
        inject.gaussian_table(100.0, step=0.125)          # 4801 nodes: above the cap
    with pytest.raises(ValueError):
        inject.normalise_peak(np.zeros(5))
    assert _native.INJECT_DTYPE == IR.TRAIL_DTYPE and _native.INJECT_DTYPE.itemsize == 48


def small_table():
    t, step = inject.gaussian_table(1.5, step=0.25, n_sigma=4.0)
    return t.astype(np.float32), step


def test_zero_amplitude_and_extents_outside_the_frame_change_no_bit():
    T, step = small_table()
    f = np.random.default_rng(1).normal(0, 1, (1, 40, 56)).astype(np.float32)
    f[0, 3, 4], f[0, 5, 6] = np.float32(-0.0), np.inf
    f.view(np.uint32)[0, 7, 8] = 0x7FC00123
    f[0, 20, :] = np.float32(-0.0)
    before = bits(f).copy()
    for tr in (IR.trail(0, 0, 20.0, 0.3, amplitude=0.0), IR.trail(0, 0, 20.0, 0.3, t0=500.0, t1=600.0),
               IR.trail(0, 0, 20.0, 0.3, t0=-700.0, t1=-600.0), IR.trail(0, 0, 1000.0, 0.3), IR.trail(0, 0, -300.0, 1.0)):
        for full in (False, True):
            IR.inject(f, [tr], T, step, 4, full=full)
            assert np.array_equal(bits(f), before)


def test_the_near_line_shortcut_changes_nothing():
    T, step = small_table()
    base = np.random.default_rng(2).normal(0, 1, (1, 37, 53)).astype(np.float32)
    for theta in (0.0, 0.4, math.pi / 2, 2.2, float(np.float32(math.pi))):
        tr = IR.trail(0, 0, 26.0 * math.cos(theta) + 18.0 * math.sin(theta), theta, amplitude=0.7)
        a = IR.inject(base.copy(), [tr], T, step, 3)
        b = IR.inject(base.copy(), [tr], T, step, 3, full=True)
        assert np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(a), bits(base))


def test_theta_zero_and_half_pi_by_hand():
    T, step = small_table()
    H, W = 24, 40
    # theta = 0: x = rho.  Every row is the same, and with rho on a pixel centre the columns are symmetric about it.
    z = np.zeros((1, H, W), np.float32)
    a = IR.inject(z.copy(), [IR.trail(0, 0, 17.0, 0.0, amplitude=2.0)], T, step, 4)[0]
    assert (a == a[0]).all() and a[0, 17] > 0
    assert np.array_equal(a[0, 17 - 8:17], a[0, 17 + 8:17:-1])
    assert not a[0, :17 - 8].any()                        # the table ends 6 px from the line
    # subsample 1 samples the pixel centre: the table itself where a node falls on it (offsets of whole px = 4 steps)
    c = IR.inject(z.copy(), [IR.trail(0, 0, 17.0, 0.0, amplitude=2.0)], T, step, 1)[0]
    M = (len(T) - 1) // 2
    for d in range(-5, 6):
        assert c[0, 17 + d] == np.float32(2.0 * float(T[M + 4 * d]))
    # theta = pi/2: y = rho in the flipped frame, buffer row H-1-rho; the same numbers transposed (cos(pi/2) = 6e-17 moves u by
    # less than 1e-14 px, which can still change the last bit of a float32 weight: the comparison is relative, and exact
    # equality with the theta = 0 numbers is not expected)
    b = IR.inject(np.zeros((1, W, H), np.float32), [IR.trail(0, 0, 17.0, math.pi / 2, amplitude=2.0)], T, step, 1)[0]
    assert np.allclose(b[::-1].T, c, rtol=1e-6, atol=0) and (b.T == b.T[0]).all()
    assert b[W - 1 - 17, 0] == c[0, 17]


def test_crossing_trails_equal_successive_calls_and_order_matters():
    T, step = small_table()
    base = np.random.default_rng(3).normal(0, 1, (1, 48, 64)).astype(np.float32)
    t1 = IR.trail(0, 0, 32 * math.cos(0.5) + 24 * math.sin(0.5), 0.5, amplitude=0.3)
    t2 = IR.trail(0, 0, 32 * math.cos(2.0) + 24 * math.sin(2.0), 2.0, amplitude=1e-3)
    both = IR.inject(base.copy(), [t1, t2], T, step, 4)
    seq = IR.inject(IR.inject(base.copy(), [t1], T, step, 4), [t2], T, step, 4)
    assert np.array_equal(bits(both), bits(seq))
    rev = IR.inject(base.copy(), [t2, t1], T, step, 4)
    assert np.allclose(both, rev, atol=1e-6) and not np.array_equal(bits(both), bits(rev))   # float32 addition does not associate


def test_a_clipped_trail_ends_within_a_pixel_of_its_end_points():
    T, step = small_table()
    H, W = 80, 96
    theta, t0, t1 = 0.6, -20.25, 14.5
    rho = 48 * math.cos(theta) + 40 * math.sin(theta)
    a = IR.inject(np.zeros((1, H, W), np.float32), [IR.trail(0, 0, rho, theta, t0=t0, t1=t1)], T, step, 4)[0]
    r, x = np.nonzero(a)
    y = H - 1 - r
    c, s = math.cos(theta), math.sin(theta)
    t = (x - rho * c) * -s + (y - rho * s) * c
    # a pixel's sample points lie within sqrt(1/2) px of its centre: nothing is added beyond the window by more than that,
    # and the pixels on the line reach each end to within a pixel
    assert t.min() >= t0 - math.sqrt(0.5) and t.max() <= t1 + math.sqrt(0.5)
    on_line = np.abs(x * c + y * s - rho) <= 0.5
    assert t[on_line].min() <= t0 + 1.0 and t[on_line].max() >= t1 - 1.0


@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("theta", [0.0, 0.3, 1.1])
def test_flux_per_unit_length(ss, theta):
    """Along a full-frame trail the added flux per unit length is amplitude x the table's trapezoid integral.  The frame's sum
    is a Riemann sum of the piecewise-linear profile P(u) over a lattice of spacing 1/ss; along the line every sample row is
    complete in the interior, so per unit length it is sum over lattice lines of P(u_i) / ss (theta = 0), the rectangle rule
    with step d = 1/ss (for other angles the lattice's projection on the normal is finer, never coarser).  For a piecewise-linear
    function with |P''| concentrated at the nodes, the rectangle rule's error is at most (d^2 / 8) * total variation of P',
    where TV(P') <= 4 max|P'| for a single-peaked table; plus float32 rounding of every addend, 2^-24 relative each."""
    T, step = inject.gaussian_table(1.5, step=0.25, n_sigma=5.0)
    T32 = T.astype(np.float32)
    amp = 3.0
    H, W = 200, 200
    rho = 100 * math.cos(theta) + 100 * math.sin(theta)
    a = IR.inject(np.zeros((1, H, W), np.float32), [IR.trail(0, 0, rho, theta, amplitude=amp)], T32, step, ss)[0].astype(np.float64)
    # the flux between two cuts across the trail, 100 px apart along it, well inside the frame: whole pixels are assigned by
    # their centre, which moves at most the band's width x sqrt(1/2) px of length across each cut
    yy, xx = np.mgrid[0:H, 0:W]
    y = H - 1 - yy
    c, s = math.cos(theta), math.sin(theta)
    t = (xx - rho * c) * -s + (y - rho * s) * c
    tm = 100 * -s + 100 * c
    got = a[(t >= tm - 50) & (t < tm + 50)].sum() / 100.0
    want = amp * inject.integral(T32.astype(np.float64), step)
    slope = np.abs(np.diff(T32.astype(np.float64))).max() / step
    quad = (1.0 / ss) ** 2 / 8 * 4 * slope * amp
    cuts = 2 * math.sqrt(0.5) * amp * float(T32.max()) * (2 * 5.0 * 1.5 + 1) / 100.0 if theta else 0.0
    assert abs(got - want) <= quad + cuts + 2.0 ** -23 * want, (got, want, quad, cuts)


def test_draw_trails_is_deterministic_and_its_checksum_is_committed():
    with open(os.path.join(GOLDEN, "inject_plan.json")) as f:
        gold = json.load(f)
    shape = tuple(gold["shape"])
    plan = recovery.draw_trails(gold["n_frames"], shape, gold["seed"], [synth.BRIGHT_PEAK])
    again = recovery.draw_trails(gold["n_frames"], shape, gold["seed"], [synth.BRIGHT_PEAK])
    assert plan.tobytes() == again.tobytes()
    assert recovery.plan_checksum(plan) == gold["sha256"]
    assert (plan["theta"] == plan["theta"].astype(np.float32).astype(np.float64)).all()
    assert ((plan["theta"] >= 0) & (plan["theta"] < math.pi)).all()
    # every line passes through the middle half of the frame
    for p in plan:
        ta, tb = recovery.extent(p["rho"], p["theta"], p["t0"], p["t1"], shape)
        assert tb - ta >= min(shape) / 2
    short = recovery.draw_trails(8, shape, 3, [0.1, 0.2], length=300.0)
    assert np.allclose(short["t1"] - short["t0"], 300.0) and list(short["peak"][:3]) == [0.1, 0.2, 0.1]
    c, s = recovery.cos_sin(np.linspace(0, math.pi, 1001))
    assert np.abs(c - np.cos(np.linspace(0, math.pi, 1001))).max() < 1e-15 and np.abs(s - np.sin(np.linspace(0, math.pi, 1001))).max() < 1e-15


def _rec(found, rho, theta):
    r = np.zeros(1, _native.RESULT_DTYPE)
    r["found"], r["rho"], r["theta"] = found, rho, theta
    return r


def test_match_on_both_sides_of_each_tolerance():
    pb, pd = {"houghMethod": 20}, {"houghMethod": 10}
    shape = (1000, 1000)
    # theta = pi/2: the line y = 400; its extent's middle is (499.5, 400); a detected line of the same angle at rho' is
    # 400 - rho' away
    tr = np.array([(0, 5.0, 400.0, float(np.float32(math.pi / 2)), -np.inf, np.inf)], recovery.PLAN_DTYPE)
    th = float(tr["theta"][0])

    def m(found, rho, theta, k=1.0):
        return recovery.match(_rec(found, rho, theta), tr, pb, pd, k=k, shape=shape)

    assert not m(0, 400.0, th)[0][0] and np.isnan(m(0, 400.0, th)[1][0])
    ok, d_rho, d_theta, length = m(1, 381.0, th)
    assert ok[0] and abs(d_rho[0] - 19.0) < 1e-3 and d_theta[0] == 0.0 and abs(length[0] - 999.0) < 1e-9
    assert not m(1, 379.0, th)[0][0] and m(1, 379.0, th, k=1.5)[0][0]           # 21 px: outside one bright cell, inside 1.5
    assert m(1, 419.0, th)[0][0] and not m(1, 421.0, th)[0][0]
    assert m(2, 391.0, th)[0][0] and not m(2, 389.0, th)[0][0]                  # the dim pass's own cell: 10 px
    # angle: the detected line turned about the middle point keeps d_rho = 0
    for dth, want in ((0.0170, True), (0.0179, False), (-0.0170, True), (-0.0179, False)):   # 1 degree = 0.017453
        t2 = float(np.float32(th + dth))
        rho2 = 499.5 * math.cos(t2) + 400.0 * math.sin(t2)
        ok, d_rho, d_theta, _ = m(1, rho2, t2)
        assert ok[0] == want and abs(d_rho[0]) < 1e-3 and abs(d_theta[0] - (t2 - th)) < 1e-12
    assert m(1, 499.5 * math.cos(th + 0.03) + 400.0 * math.sin(th + 0.03), th + 0.03, k=2.0)[0][0]


def test_match_folds_theta_at_zero_and_pi():
    pb = pd = {"houghMethod": 20}
    shape = (1000, 1000)
    # injected: x = 300 at theta = 0.004; detected as (-rho, theta + pi - 0.008): the same line but for 0.008 rad
    tr = np.array([(0, 5.0, 300.0, float(np.float32(0.004)), -np.inf, np.inf)], recovery.PLAN_DTYPE)
    thd = float(np.float32(math.pi - 0.004))
    # the detected line through the injected extent's middle, 5 px off along its own normal
    ta, tb = recovery.extent(300.0, float(tr["theta"][0]), -np.inf, np.inf, shape)
    c, s = math.cos(float(tr["theta"][0])), math.sin(float(tr["theta"][0]))
    tm = 0.5 * (ta + tb)
    mx, my = 300.0 * c - tm * s, 300.0 * s + tm * c
    rho_d = mx * math.cos(thd) + my * math.sin(thd) - 5.0
    assert rho_d < 0
    ok, d_rho, d_theta, _ = recovery.match(_rec(1, rho_d, thd), tr, pb, pd, k=1.0, shape=shape)
    assert ok[0] and abs(d_theta[0] - (thd - math.pi - float(tr["theta"][0]))) < 1e-12 and abs(d_rho[0] + 5.0) < 1e-3
    far = recovery.match(_rec(1, rho_d - 30.0, thd), tr, pb, pd, k=1.0, shape=shape)
    assert not far[0][0] and abs(far[1][0] + 35.0) < 1e-3
    # and the other way round: injected near pi, detected near 0
    tr2 = np.array([(0, 5.0, rho_d + 5.0, thd, -np.inf, np.inf)], recovery.PLAN_DTYPE)
    ok, d_rho, d_theta, _ = recovery.match(_rec(1, 300.0, float(tr["theta"][0])), tr2, pb, pd, k=1.0, shape=shape)
    assert ok[0] and d_theta[0] > 0 and abs(d_theta[0] - 0.008) < 1e-6 and abs(d_rho[0]) < 1e-2


def test_completeness_against_hand_computed_wilson_intervals():
    rows = np.zeros(14, recovery.ROW_DTYPE)
    rows["peak"] = [0.1] * 4 + [0.2] * 10
    rows["matched"] = [1, 0, 0, 0] + [1] * 9 + [0]
    rows["found"] = [1, 1, 0, 0] + [1] * 10
    tab = recovery.completeness(rows, [0.0, 0.15, 0.25, 1.0])
    assert [(b["n"], b["recovered"]) for b in tab] == [(4, 1), (10, 9), (0, 0)]
    # z = 1, n = 4, p = 1/4: centre (0.25 + 1/8) / (1 + 1/4) = 0.3; half = sqrt(0.25 * 0.75 / 4 + 1/64) / 1.25 = 0.2
    assert abs(tab[0]["efficiency"] - 0.25) < 1e-15 and abs(tab[0]["wilson_lo"] - 0.1) < 1e-12 and abs(tab[0]["wilson_hi"] - 0.5) < 1e-12
    # z = 1, n = 10, p = 0.9: centre (0.9 + 0.05) / 1.1; half = sqrt(0.009 + 0.0025) / 1.1
    mid, half = 0.95 / 1.1, math.sqrt(0.0115) / 1.1
    assert abs(tab[1]["wilson_lo"] - (mid - half)) < 1e-12 and abs(tab[1]["wilson_hi"] - (mid + half)) < 1e-12
    assert math.isnan(tab[2]["efficiency"]) and math.isnan(tab[2]["wilson_lo"])
    # z = 2, n = 4, p = 1/2: centre 1/2, half = 2 sqrt(1/16 + 1/16) / 2 = sqrt(1/8)
    lo, hi = recovery.wilson(2, 4, z=2.0)
    assert abs(lo - (0.5 - math.sqrt(0.125))) < 1e-12 and abs(hi - (0.5 + math.sqrt(0.125))) < 1e-12
    assert recovery.peak_edges([0.2, 0.1, 0.2, 5]) == [0.0, 0.15000000000000002, 2.6, math.inf]


def test_recovery_text_round_trip(tmp_path):
    rows = np.zeros(3, recovery.ROW_DTYPE)
    rows["frame"] = [0, 1, 7]
    rows["peak"] = [0.1, 1 / 3, 5.0]
    rows["rho"] = [-311.4442788402734, 1e-300, 2.5]
    rows["theta"] = [float(np.float32(2.76)), 0.0, math.pi]
    rows["length"] = [412.49, 0.0, 2000.0]
    rows["found"], rows["matched"] = [1, 0, 2], [1, 0, 0]
    rows["d_rho"], rows["d_theta"] = [13.98, np.nan, -4.0], [0.0139, np.nan, -1e-9]
    rows["fwhm"] = [4.7, np.nan, np.nan]
    p = tmp_path / "recovery.txt"
    recovery.write_recovery(p, rows)
    back = recovery.read_recovery(p)
    assert back.dtype == rows.dtype and back.tobytes() == rows.tobytes()
    with open(p) as f:
        assert f.readline().split() == list(recovery.ROW_COLUMNS) and len(f.readlines()) == 3


def test_recovery_chain_on_the_cpu_gives_the_committed_rows(oracle):
    """the 16-frame set injected with the restatement and detected with the oracle: the committed rows, and the chain condition
    (at BRIGHT_PEAK every trail of the set is recovered and matched)"""
    sys.path.insert(0, GOLDEN)
    import make_inject_recovery
    with open(os.path.join(GOLDEN, "inject_recovery.json")) as f:
        gold = json.load(f)
    rows, plan = make_inject_recovery.cpu_rows()
    assert gold["k"] == recovery.K_MATCH
    assert IR.rows_to_json(rows) == gold["rows"]
    assert len(rows) == 16 and (rows["peak"] == synth.BRIGHT_PEAK).all()
    assert (rows["found"] != 0).all() and rows["matched"].all()


def test_recovery_never_imports_tests_or_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("inject.py", "recovery.py"):
        with open(os.path.join(root, "lfd_amd", name)) as f:
            text = f.read()
        assert "inject_ref" not in text and "import oracle" not in text and "from oracle" not in text and "from tests" not in text
