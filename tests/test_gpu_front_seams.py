"""The front end of a pass at the seams of its kernels: every case of tests/front_cases.py through lfdmi_process_bright,
lfdmi_process_dim and lfdmi_detect_batch, without and with the 8-bit stage images (the two modes take different kernels), and
every stage image the call leaves compared bit for bit with the oracle's operators applied one after the other.  A failure
names the case, the route, the stage, the number of differing pixels and the first of them."""
import numpy as np
import pytest

import front_cases as fc
from front_cases import CASES, BY_NAME

pytestmark = pytest.mark.gpu

ENTRY_DIM = {"bright": False, "dim": True, "batch": True}
_refs = {}


def stage_ids():
    from lfd_amd import _native
    return dict(GRAY=_native.STAGE_GRAY, EQU=_native.STAGE_EQU, CANNY=_native.STAGE_CANNY, BOX=_native.STAGE_BOX, ERODED=_native.STAGE_ERODED,
                EQUALIZED=_native.STAGE_EQUALIZED)


def reference(O, key, frame, params, entry):
    """The stage images and the oracle's record for one frame (computed once, shared, never written to)."""
    if key not in _refs:
        p = params[1] if entry == "batch" else params
        r = fc.reference(O, frame, p, ENTRY_DIM[entry])
        raw = np.ascontiguousarray(frame[::-1])
        if entry == "bright":
            r["record"] = O.process_bright(raw, p, flip=True)
        elif entry == "dim":
            r["record"] = O.process_dim(raw, p, flip=True, after_bright=True)
        else:
            r["record"] = O.detect_frame(raw.copy(), params[0], params[1])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def run(ctx, entry, params, frames):
    """frames [n, h, w] as the kernels should see them -> the n records."""
    raw = np.ascontiguousarray(frames[:, ::-1])
    if entry == "bright":
        return ctx.process_bright(raw, params, flip=True)[0]
    if entry == "dim":
        return ctx.process_dim(raw, params, flip=True, after_bright=True)[0]
    return ctx.detect_batch(raw, params[0], params[1])


def check_record(got, want, what):
    bad = {k: (got[k].item(), v) for k, v in want.items() if got[k].item() != v}
    assert not bad, f"{what}: record differs from the oracle's (device, oracle): {bad}"


def check_images(ctx, slot, ref, rt, shape, what):
    """Every stage image the route leaves, and the number of rectangles fit_minAreaRect accepted (C_NQUADS: two per ring where
    the hole border passes lwTresh too, so a hole that is lost shows even where its rectangle lies inside its ring's)."""
    h, w = shape
    ids = stage_ids()
    quads = int(ctx.get_counters(slot, 1)[0, fc.C_NQUADS])
    assert quads == ref["n_boxes"], f"{what}: {quads} accepted rectangles on the device, {ref['n_boxes']} in the oracle"
    for st in rt["fetch"]:
        got, want = ctx.get_stage(slot, ids[st], h, w), ref[st]
        if st in ("CANNY", "BOX"):
            got, want = got != 0, want != 0
        bad = got != want
        if bad.any():
            y, x = (int(v) for v in np.argwhere(bad)[0])
            route = {k: v for k, v in rt.items() if k != "fetch"}
            pytest.fail(f"{what}, route {route}: stage {st}: {int(bad.sum())} pixels differ, first at (row {y}, column {x}): "
                        f"device {int(got[y, x])}, oracle {int(want[y, x])}")


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_stage_images_at_the_seam(oracle, monkeypatch, c):
    from lfd_amd import _native
    for k, v in c.knobs.items():
        monkeypatch.setenv(k, v)
    h, w = c.frame.shape
    for entry in c.entries:
        params = c.params(entry)
        ref = reference(oracle, (c.name, entry), c.frame, params, entry)
        for mode in (0, 1):
            rt = fc.route(h, w, params[1] if entry == "batch" else params, entry, mode, c.knobs)
            what = f"{c.name} / {entry} / stage images {mode}"
            with _native.Context(0, h, w, 1) as ctx:
                ctx.set_stage_images(mode)
                rec = run(ctx, entry, params, c.frame[None])
                check_record(rec[0], ref["record"], what)
                check_images(ctx, 0, ref, rt, (h, w), what)
                if c.ntiles is not None and entry == "bright" and rt["dc"] == "tiles":
                    assert int(ctx.get_counters(0, 1)[0, fc.C_NTILES]) == c.ntiles, what
                if rt["front"] == "bits" and rt["dc"] == "tiles":
                    # k_bits_erode marks the cells of its survivors: the tile list is the one of the eroded image, no longer
                    want = int(fc.active_tiles(ref["ERODED"]).sum())
                    assert int(ctx.get_counters(0, 1)[0, fc.C_NTILES]) == want, f"{what}: tiles listed"


def test_label_table_one_run_short_exact_and_one_to_spare(oracle, monkeypatch):
    """LFDMI_FRAME_RUNCAP at R - 1, R and R + 1 for a frame with R candidate runs (k_frame_fg keeps a frame with nrun <= cap),
    and at B - 1, B and B + 1 for its B background runs (k_frame_contours keeps it with both counts <= cap): same images
    whichever kernels take the frame.  Which took it is observed, not assumed: a frame either kernel hands to the general
    ones makes the context run the chunk again (stats()["general_reruns"]), so the count is 1 below max(R, B) and 0 from there."""
    from lfd_amd import _native
    c = BY_NAME[fc.RUNCAP_CASE]
    h, w = c.frame.shape
    for entry in ("bright", "dim"):
        params = c.params(entry)
        ref = reference(oracle, (c.name, entry), c.frame, params, entry)
        rt = fc.route(h, w, params, entry, 0)
        with _native.Context(0, h, w, 1) as ctx:
            ctx.set_stage_images(0)
            run(ctx, entry, params, c.frame[None])
            R, B = (int(v) for v in ctx.get_counters(0, 1)[0, [fc.C_NRUNF, fc.C_NRUNB]])
            assert ctx.stats()["general_reruns"] == 0
        assert 8 < R < fc.FRAME_RUNCAP and 8 < B < fc.FRAME_RUNCAP, (R, B)
        for cap in sorted({R - 1, R, R + 1, B - 1, B, B + 1}):
            monkeypatch.setenv("LFDMI_FRAME_RUNCAP", str(cap))
            what = f"{c.name} / {entry} / LFDMI_FRAME_RUNCAP={cap} of {R} candidate and {B} background runs"
            with _native.Context(0, h, w, 1) as ctx:
                ctx.set_stage_images(0)
                rec = run(ctx, entry, params, c.frame[None])
                check_record(rec[0], ref["record"], what)
                check_images(ctx, 0, ref, rt, (h, w), what)
                assert int(ctx.get_counters(0, 1)[0, fc.C_NRUNF]) == R, what
                assert ctx.stats()["general_reruns"] == (1 if cap < max(R, B) else 0), (what, ctx.stats())


@pytest.mark.parametrize("name,entry", fc.SEQUENCE_CASES)
def test_three_frames_through_two_slots_then_another_call(oracle, name, entry):
    """Two chunks (2 + 1 frames) on one context, then a second call with another frame: every record, the images of the last
    chunk's slot, and after the second call nothing of the first shows through (planes that are only partly rewritten)."""
    from lfd_amd import _native
    c = BY_NAME[name]
    for k, v in c.knobs.items():
        assert v == "1", "default knobs only: the cases of this test run without a monkeypatch"
    h, w = c.frame.shape
    frames = np.stack([c.frame, np.roll(c.frame, (5, 37), (0, 1)), c.frame[::-1, ::-1]])
    params = c.params(entry)
    refs = [reference(oracle, (c.name, entry, "seq", i), frames[i], params, entry) for i in range(3)]
    for mode in (0, 1):
        rt = fc.route(h, w, params[1] if entry == "batch" else params, entry, mode, c.knobs)
        with _native.Context(0, h, w, 2) as ctx:
            ctx.set_stage_images(mode)
            recs = run(ctx, entry, params, frames)
            for i in range(3):
                check_record(recs[i], refs[i]["record"], f"{name} / {entry} / mode {mode} / frame {i} of 3")
            check_images(ctx, 0, refs[2], rt, (h, w), f"{name} / {entry} / mode {mode} / second chunk")
            recs = run(ctx, entry, params, frames[1:2])
            check_record(recs[0], refs[1]["record"], f"{name} / {entry} / mode {mode} / second call")
            check_images(ctx, 0, refs[1], rt, (h, w), f"{name} / {entry} / mode {mode} / second call")


def streak_frame():
    f = fc.blank(80, 448, 70)
    yy, xx = np.mgrid[0:80, 0:448]
    f[np.abs(yy - (0.12 * xx + 8)) < 2.0] = fc.AMPS[3]
    return f


def test_six_reach_cases_and_two_decided_frames_in_an_eight_slot_batch(oracle):
    """One lfdmi_detect_batch of eight 80 x 448 frames: a reach case in six slots and, in slots 1 and 4, a streak the bright pass
    already decides (their dim images do not exist and are not compared), so the dim pass works on a subset of the slots through
    the permutation of the active slots (k_active_perm).  Without and with the stage images.  k_tile_perm needs more than eight
    frames and is not reached here."""
    from lfd_amd import _native
    pb, pd = fc.default_params()
    sides = list(fc.REACH_SPOTS)
    frames, names = [], []
    for i in range(8):
        if i in (1, 4):
            frames.append(streak_frame()); names.append("streak")
        else:
            frames.append(BY_NAME[f"reach_{sides[i]}"].frame); names.append(f"reach_{sides[i]}")
    frames = np.stack(frames)
    refs = [reference(oracle, (names[i], "batch8"), frames[i], (pb, pd), "batch") for i in range(8)]
    assert [r["record"]["found"] for r in refs] == [0, 1, 0, 0, 1, 0, 0, 0]
    for mode in (0, 1):
        rt = fc.route(80, 448, pd, "batch", mode)
        assert rt["front"] == ("erode" if mode else "bits") and rt["dc"] == "tiles"
        with _native.Context(0, 80, 448, 8) as ctx:
            ctx.set_stage_images(mode)
            recs = run(ctx, "batch", (pb, pd), frames)
            for i in range(8):
                check_record(recs[i], refs[i]["record"], f"slot {i} ({names[i]}) / mode {mode}")
                if names[i] != "streak":
                    check_images(ctx, i, refs[i], rt, (80, 448), f"slot {i} ({names[i]}) of an 8-slot batch / mode {mode}")
