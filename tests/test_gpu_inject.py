"""Trail injection on the device against the numpy restatement of include/lfdmi.h (tests/inject_ref.py): bit for bit over
shapes, angles, extents, sub-samplings, crossing trails, special pixel values and the three frame locations; the refusals; the
recovery chain against the committed CPU rows; the defocus fit of injected model trails; a 256-frame device batch."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PI32 = float(np.float32(math.pi))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{len(bad)} pixels differ, first at {i}: device {got[i]!r} ({g[i]:#x}), restatement {want[i]!r} ({w[i]:#x})")


def tables():
    """two tables of one length: a Gaussian (sigma 2 px, peak 1) and an asymmetric ramp with a dip"""
    from lfd_amd import inject
    g, step = inject.gaussian_table(2.0, step=0.25, n_sigma=5.0)
    k = np.arange(len(g), dtype=np.float64)
    ramp = (k / len(g)) * (1.0 + 0.5 * np.sin(k * 0.37)) * (np.abs(k - len(g) // 2) > 3)
    return np.stack([g, ramp]).astype(np.float32), step


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.025, shape).astype(np.float32)


def through(shape, x, y, theta):
    """rho of the line of angle theta through the point (x, y) of the flipped frame"""
    return x * math.cos(theta) + y * math.sin(theta)


def along(x, y, theta):
    """t of the point (x, y) on the line of angle theta through it"""
    rho = x * math.cos(theta) + y * math.sin(theta)
    return (x - rho * math.cos(theta)) * -math.sin(theta) + (y - rho * math.sin(theta)) * math.cos(theta)


def edge_cases(shape):
    """trails (frame 0, table 0) leaving through every edge and corner, both signs of rho, bounded and unbounded"""
    h, w = shape
    tr = []
    for theta in (0.0, math.pi / 2, PI32, 0.35, 1.2, 2.4, 3.0, float(np.float32(0.7853982))):
        rho = through(shape, w / 2 + 3.25, h / 2 - 1.5, theta)
        tr.append(IR.trail(0, 0, rho, theta, amplitude=0.5))
    tr.append(IR.trail(0, 1, through(shape, 0.0, 0.0, 2.3), 2.3, amplitude=0.25))                  # through the corner (0, 0)
    tr.append(IR.trail(0, 0, through(shape, w - 1.0, h - 1.0, 2.4), 2.4, amplitude=0.25))          # and the opposite one
    tr.append(IR.trail(0, 1, through(shape, w - 1.0, 0.0, 0.8), 0.8, amplitude=0.25))
    tr.append(IR.trail(0, 0, through(shape, 0.0, h - 1.0, 0.75), 0.75, amplitude=0.25))
    tr.append(IR.trail(0, 0, 1.5, 0.0, amplitude=1.0))                                             # along the left edge
    tr.append(IR.trail(0, 0, -(h - 2.25), 3 * math.pi / 2 - 1e-3, amplitude=1.0))                  # negative rho, near the top row
    tm = along(w / 3, h / 3, 1.0)
    tr.append(IR.trail(0, 1, through(shape, w / 3, h / 3, 1.0), 1.0, t0=tm - 40.5, t1=tm + 55.25, amplitude=2.0))   # bounded both sides
    tm = along(w / 3, h / 2, 2.0)
    tr.append(IR.trail(0, 0, through(shape, w / 3, h / 2, 2.0), 2.0, t0=tm - 10.0, amplitude=-1.0))   # bounded on one side, negative
    return np.array(tr, IR.TRAIL_DTYPE)


@pytest.fixture(scope="module")
def ctx():
    from lfd_amd import _native
    c = _native.Context(0, 1489, 2048, 8)
    yield c
    c.close()


@pytest.mark.parametrize("shape", [(384, 640), (157, 333)])
@pytest.mark.parametrize("ss", [1, 4, 8])
def test_every_edge_angle_and_extent_equals_the_restatement(ctx, shape, ss):
    tabs, step = tables()
    cases = edge_cases(shape)
    frames = noise((len(cases), *shape), 3)
    tr = cases.copy()
    tr["frame"] = np.arange(len(cases))
    want = IR.inject(frames.copy(), tr, tabs, step, ss)
    got = ctx.inject_trails(frames.copy(), tr, tabs, step, subsample=ss)
    assert_same_bits(got, want)
    assert not np.array_equal(bits(got), bits(frames))


def special_frames(shape, seed):
    f = noise(shape, seed)
    flat = f.reshape(f.shape[0], -1)
    rng = np.random.default_rng(seed + 1)
    idx = rng.integers(0, flat.shape[1], (f.shape[0], 4000))
    for i in range(f.shape[0]):
        flat[i, idx[i, :1000]] = np.float32(-0.0)
        flat[i, idx[i, 1000:2000]] = np.inf
        flat[i, idx[i, 2000:3000]] = -np.inf
        flat.view(np.uint32)[i, idx[i, 3000:]] = np.uint32(0x7FC12345)     # NaN with a payload
    return f


def sdss_case():
    """1489 x 2048: 5 frames; frame 1 carries three trails, two of them crossing; frames 2 and 4 none"""
    shape = (1489, 2048)
    h, w = shape
    tr = [IR.trail(0, 0, through(shape, 1000.0, 700.0, 0.35), 0.35, amplitude=0.05),
          IR.trail(1, 0, through(shape, 1024.0, 744.0, 1.2), 1.2, amplitude=0.3),
          IR.trail(3, 1, through(shape, 300.0, 1200.0, PI32), PI32, amplitude=0.2),
          IR.trail(1, 1, through(shape, 1024.0, 744.0, 2.4), 2.4, amplitude=0.2),                  # crosses the first of frame 1
          IR.trail(1, 0, through(shape, 1500.0, 300.0, 1.25), 1.25, t0=along(1500.0, 300.0, 1.25) - 300.0,
                   t1=along(1500.0, 300.0, 1.25) + 100.0, amplitude=1.0),
          IR.trail(3, 0, -5000.0, 0.5, amplitude=1.0)]                                             # never reaches the frame
    return shape, np.array(tr, IR.TRAIL_DTYPE), 5


def test_sdss_frames_crossing_trails_and_special_pixels_in_every_location(ctx):
    import torch
    shape, tr, n = sdss_case()
    tabs, step = tables()
    frames = special_frames((n, *shape), 11)
    want = IR.inject(frames.copy(), tr, tabs, step, 4)
    assert np.array_equal(bits(want[2]), bits(frames[2])) and np.array_equal(bits(want[4]), bits(frames[4]))
    # host
    got = ctx.inject_trails(frames.copy(), tr, tabs, step)
    assert_same_bits(got, want)
    # device
    dev = torch.from_numpy(frames.copy()).cuda()
    ctx.inject_trails(dev, tr, tabs, step)
    assert_same_bits(dev.cpu().numpy(), want)
    # pinned
    buf = ctx.pinned_buffer(frames.nbytes)
    pin = buf.array.view(np.float32).reshape(frames.shape)
    pin[...] = frames
    ctx.inject_trails(pin, tr, tabs, step, pinned=True)
    assert_same_bits(pin, want)
    del pin
    buf.close()
    # the two crossing trails of frame 1 in one call equal two successive calls
    one = torch.from_numpy(frames[1:2].copy()).cuda()
    for t in tr[tr["frame"] == 1]:
        t = t.copy()
        t["frame"] = 0
        ctx.inject_trails(one, np.array([t]), tabs, step)
    assert_same_bits(one.cpu().numpy()[0], want[1])


def test_refusals_leave_the_context_usable(ctx):
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    tabs, step = tables()
    shape = (64, 96)
    frames = noise((2, *shape), 5)
    good = np.array([IR.trail(1, 0, 40.0, 0.3)], IR.TRAIL_DTYPE)

    def refused(fr, tr, tb, st=step, ss=4):
        before = fr.copy() if isinstance(fr, np.ndarray) else None
        with pytest.raises(_native.NativeError) as e:
            ctx.inject_trails(fr, tr, tb, st, subsample=ss)
        assert e.value.code == _native.ERR_ARG
        if before is not None:
            assert np.array_equal(bits(fr), bits(before))

    refused(frames.astype(">f4"), good, tabs)                                     # LFDMI_F32_BE
    for f in (-1, 2):
        bad = good.copy()
        bad["frame"] = f
        refused(frames, bad, tabs)
    for t in (-1, 2):
        bad = good.copy()
        bad["table"] = t
        refused(frames, bad, tabs)
    refused(frames, good, tabs[:, :-1])                                           # even table_len
    refused(frames, good, np.zeros((1, _native.INJECT_MAX_TABLE + 2), np.float32))  # above the cap
    refused(frames, good, tabs, ss=0)
    refused(frames, good, tabs, ss=9)
    refused(frames, good, tabs, st=0.0)
    for field in ("rho", "theta", "amplitude"):
        bad = good.copy()
        bad[field] = np.nan
        refused(frames, bad, tabs)
    # a table at the cap is taken
    big = np.ones((1, _native.INJECT_MAX_TABLE), np.float32)
    want = IR.inject(frames.copy(), good, big, 0.01, 2)
    assert_same_bits(ctx.inject_trails(frames.copy(), good, big, 0.01, subsample=2), want)
    # while a detect_batch_begin is in flight
    pb, pd, _ = default_params()
    dev = torch.from_numpy(noise((2, 384, 640), 6)).cuda()
    with _native.Context(0, 384, 640, 2) as c2:
        pend = c2.detect_batch_begin(dev, pb, pd)
        other = torch.from_numpy(frames.copy()).cuda()
        with pytest.raises(_native.NativeError):
            c2.inject_trails(other, good, tabs, step)
        pend.result()
        assert np.array_equal(bits(other.cpu().numpy()), bits(frames))
        c2.inject_trails(other, good, tabs, step)
        assert_same_bits(other.cpu().numpy(), IR.inject(frames.copy(), good, tabs, step, 4))
    # and the module's context still works after every refusal
    assert_same_bits(ctx.inject_trails(frames.copy(), good, tabs, step), IR.inject(frames.copy(), good, tabs, step, 4))


def test_host_frames_in_more_than_one_staging_chunk(ctx):
    """host frames are staged at most 512 MiB at a time: 41 SDSS frames; 46 frames that all carry a trail take two chunks, whose
    frames share the staging buffer's slots, and frames without a trail between them take none"""
    shape = (1489, 2048)
    tabs, step = tables()
    n = 50
    carrying = [f for f in range(n) if f % 13 != 5]
    assert len(carrying) == 46 and len(carrying) * shape[0] * shape[1] * 4 > 512 << 20
    frames = np.zeros((n, *shape), np.float32)
    frames[:, ::7, ::5] = np.float32(-0.0)
    tr = []
    for f in carrying:
        theta = 0.1 + 0.06 * f
        x, y = 300.0 + 29 * f, 200.0 + 21 * f
        tm = along(x, y, theta)
        tr.append(IR.trail(f, f % 2, through(shape, x, y, theta), theta, t0=tm - 60.0, t1=tm + 45.5, amplitude=0.5 + f))
    tr = np.array(tr, IR.TRAIL_DTYPE)
    want = IR.inject(frames.copy(), tr, tabs, step, 2)
    got = ctx.inject_trails(frames.copy(), tr, tabs, step, subsample=2)
    assert_same_bits(got, want)
    assert all(want[f].any() for f in carrying) and not any(want[f].any() for f in range(n) if f not in carrying)


def test_recovery_chain_gives_the_committed_rows():
    """injection is bit-equal to the restatement and detection to the oracle, so recovery.run on the device gives exactly the
    rows the CPU chain wrote into tests/golden/inject_recovery.json"""
    from lfd_amd import _native, recovery
    from lfd_amd.detecttrails import default_params
    with open(os.path.join(GOLDEN, "inject_recovery.json")) as f:
        gold = json.load(f)["rows"]
    with open(os.path.join(GOLDEN, "inject_plan.json")) as f:
        plan_gold = json.load(f)
    frames, cats, plan, table, step = IR.recovery_set()
    assert recovery.plan_checksum(plan) == plan_gold["sha256"]
    pb, pd, prs = default_params()
    rs = _native.make_rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    with _native.Context(0, *IR.SET_SHAPE, 16) as c:
        rows = recovery.run(c, frames, cats, rs, plan, table, step, pb, pd)
        assert IR.rows_to_json(rows) == gold
        assert rows["matched"].all()
        withp = recovery.run(c, frames, cats, rs, plan, table, step, pb, pd, profiles=True)
    assert np.array_equal(withp["matched"], rows["matched"])
    # a Gaussian of sigma 2 px seen through the pixel: FWHM 4.7 px; calc_fwhm reads low by up to 2 bins of 0.1 px
    assert np.isfinite(withp["fwhm"]).all() and (np.abs(withp["fwhm"] - 4.75) < 0.6).all(), withp["fwhm"]


def test_defocus_fit_of_injected_model_trails():
    """defocus_table(100 km) and the focus table, normalised to 2 sky sigmas, injected into pure noise at the three angles of
    test_gpu_defocus.test_recovery_of_rendered_trails; measure_trails and fit_defocus with the default bank plus the true
    height give h within the 10 % that test allows its numpy renderer, and the focus table the focus model."""
    from lfd_amd import _native, defocus, inject
    angles = (0.35, 1.2, 2.4)
    shape = (1489, 2048)
    tabs, steps = zip(*[inject.defocus_table(h) for h in (100.0, np.inf)])
    assert steps[0] == steps[1]
    L = max(len(t) for t in tabs)
    padded = np.zeros((2, L))
    for i, t in enumerate(tabs):
        o = (L - len(t)) // 2
        padded[i, o:o + len(t)] = inject.normalise_peak(t)
    rng = np.random.default_rng(7)
    frames = rng.normal(0.0, 1.0, (6, *shape)).astype(np.float32)
    tr = inject.make_trails(6)
    recs = np.zeros(6, _native.RESULT_DTYPE)
    for k in range(6):
        th = float(np.float32(angles[k % 3]))
        rho = float(np.float32(1024 * math.cos(th) + 744 * math.sin(th)))
        tr[k] = (k, k // 3, rho, th, -np.inf, np.inf, 2.0)
        recs[k]["found"], recs[k]["rho"], recs[k]["theta"] = 1, rho, th
    with _native.Context(0, *shape, 4) as c:
        c.inject_trails(frames, tr, padded, steps[0], subsample=8)
        trails, prof = c.measure_trails(frames, recs)
        assert (trails["status"] == _native.TRAIL_OK).all(), trails["status"]
        heights = np.union1d(defocus.default_params()["heights"], [100.0])
        with defocus.DefocusBank(c, heights=heights) as bank:
            fit = c.fit_defocus(bank, trails, prof)
            dchi = bank.delta_chi2
    report = "\n".join("table %d theta %s: h_fit %.2f [%.2f, %.2f] chi2 %.1f chi2_focus %.1f" % (
        t["table"], t["theta"], f["h_km"], f["h_lo"], f["h_hi"], f["chi2"], f["chi2_focus"]) for t, f in zip(tr, fit))
    print(report)
    for t, f in zip(tr, fit):
        assert f["status"] == _native.DEFOCUS_OK, report
        if t["table"] == 0:
            assert abs(f["h_km"] - 100.0) / 100.0 <= 0.10, report
        else:
            assert f["h_hi"] == np.inf and f["chi2_focus"] - f["chi2"] <= dchi, report


def test_a_256_frame_device_batch_equals_256_single_frame_calls():
    import torch
    from lfd_amd import _native, inject, recovery, synth
    n = 256
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.randn((n, *synth.SDSS_SHAPE), generator=g, device="cuda", dtype=torch.float32) * 0.025
    table, step = inject.gaussian_table(2.0)
    table = inject.normalise_peak(table).astype(np.float32)
    plan = recovery.draw_trails(n, synth.SDSS_SHAPE, 9, [0.05, 0.2, 5.0])
    tr = recovery.to_inject(plan)
    tr = tr[np.arange(n) % 7 != 3]                         # some frames carry no trail
    with _native.Context(0, *synth.SDSS_SHAPE, 8) as c:
        batch = base.clone()
        c.inject_trails(batch, tr, table, step)
        assert not torch.equal(batch, base)
        for f in range(n):
            one = base[f:f + 1].clone()
            t = tr[tr["frame"] == f].copy()
            t["frame"] = 0
            c.inject_trails(one, t, table, step)
            assert torch.equal(one[0].view(torch.int32), batch[f].view(torch.int32)), f
            if len(t) == 0:
                assert torch.equal(one[0].view(torch.int32), base[f].view(torch.int32))
    # one frame of the batch against the restatement
    f = int(tr["frame"][0])
    t = tr[:1].copy()
    t["frame"] = 0
    want = IR.inject(base[f:f + 1].cpu().numpy(), t, table, step, 4)
    assert_same_bits(batch[f].cpu().numpy(), want[0])
