"""k_frame_contours gives no key to a hole whose border the rectangle filter is certain to reject (LFDMI_HOLE_PRUNE, default
on): records, accepted rectangles and box images are the oracle's with the switch off and on, on frames of rings, slits, nested
rings and islands at word and tile edges; the counters show that holes were in fact dropped; a frame whose only rectangle is a
hole border's keeps it; and the same on the general kernels (LFDMI_FRAME_RUNCAP lowered) and with the hole table full."""
import numpy as np
import pytest

import front_cases as fc
import hole_cases as hc

pytestmark = pytest.mark.gpu

_refs = {}


def reference(O, name, build, entry):
    """Frame, oracle stage images and record of one case and entry (computed once, shared, never written to)."""
    if (name, entry) not in _refs:
        frame = build()
        p = fc.default_params()[entry == "dim"]
        r = fc.reference(O, frame, p, entry == "dim")
        raw = np.ascontiguousarray(frame[::-1])
        r["record"] = O.process_dim(raw, p, flip=True, after_bright=True) if entry == "dim" else O.process_bright(raw, p, flip=True)
        cs, flags = O.find_contours(r["CANNY"], O.RETR_LIST)
        r["holes"] = int(sum(flags))
        r["frame"], r["params"] = frame, p
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[(name, entry)] = r
    return _refs[(name, entry)]


def run_and_check(ctx, ref, entry, what):
    """One frame through the entry on a fresh context: record, rectangle count, edge and box image against the oracle.
    Returns the frame's counters."""
    from lfd_amd import _native
    h, w = ref["frame"].shape
    raw = np.ascontiguousarray(ref["frame"][None, ::-1])
    ctx.set_stage_images(0)
    rec = (ctx.process_dim(raw, ref["params"], flip=True, after_bright=True) if entry == "dim" else ctx.process_bright(raw, ref["params"], flip=True))[0]
    bad = {k: (rec[0][k].item(), v) for k, v in ref["record"].items() if rec[0][k].item() != v}
    assert not bad, f"{what}: record differs from the oracle's (device, oracle): {bad}"
    cnt = ctx.get_counters(0, 1)[0]
    assert int(cnt[fc.C_NQUADS]) == ref["n_boxes"], f"{what}: {int(cnt[fc.C_NQUADS])} accepted rectangles on the device, {ref['n_boxes']} in the oracle"
    for st, sid in (("CANNY", _native.STAGE_CANNY), ("BOX", _native.STAGE_BOX)):
        diff = (ctx.get_stage(0, sid, h, w) != 0) != (ref[st] != 0)
        assert not diff.any(), f"{what}: stage {st}: {int(diff.sum())} pixels differ, first at {tuple(int(v) for v in np.argwhere(diff)[0])}"
    return cnt


@pytest.mark.parametrize("name", list(hc.FRAMES))
def test_same_as_the_oracle_with_and_without_pruning(oracle, monkeypatch, name):
    from lfd_amd import _native
    for entry in ("bright", "dim"):
        ref = reference(oracle, name, hc.FRAMES[name], entry)
        h, w = ref["frame"].shape
        cnt = {}
        for prune in (0, 1):
            monkeypatch.setenv("LFDMI_HOLE_PRUNE", str(prune))
            with _native.Context(0, h, w, 1) as ctx:
                cnt[prune] = run_and_check(ctx, ref, entry, f"{name} / {entry} / LFDMI_HOLE_PRUNE={prune}")
                assert ctx.stats()["general_reruns"] == 0
        print(name, entry, "holes", ref["holes"], "counters (keys, slots, holes, pruned) off", cnt[0][[0, 1, 20, 21]], "on", cnt[1][[0, 1, 20, 21]])
        for prune in (0, 1):
            assert int(cnt[prune][hc.C_NHOLES]) == ref["holes"], (name, entry, prune)
        assert int(cnt[0][hc.C_NHOLES_PRUNED]) == 0
        pruned = int(cnt[1][hc.C_NHOLES_PRUNED])
        # every dropped hole is a key less, with its rows (at least three: a hole's border reaches one row above and below it)
        assert int(cnt[1][hc.C_NKEYS]) == int(cnt[0][hc.C_NKEYS]) - pruned
        assert int(cnt[1][hc.C_NSLOTS]) <= int(cnt[0][hc.C_NSLOTS]) - 3 * pruned
        if entry == "bright":
            assert pruned > 0 and ref["holes"] > 0, (name, "no hole was rejected: the case does not test what it is named for")
            if name.startswith("mixed"):
                assert 0 < pruned < ref["holes"], (name, pruned, ref["holes"])


@pytest.mark.parametrize("name", ["slit_in_blob_64x192", "slit_in_blob_130x257"])
def test_rectangle_of_a_hole_border_alone_is_kept(oracle, monkeypatch, name):
    """The frame's one accepted rectangle is a hole border's (the oracle's contours say so), beside a hole that is dropped."""
    from lfd_amd import _native
    ref = reference(oracle, name, hc.FRAMES[name], "bright")
    p = ref["params"]
    cs, flags = oracle.find_contours(ref["CANNY"], oracle.RETR_LIST)
    accepted = []
    for c, hole in zip(cs, flags):
        rect = oracle.min_area_rect(c)
        length, width = max(rect[2], rect[3]), min(rect[2], rect[3])
        if length > p["minAreaRectMinLen"] and width > p["minAreaRectMinLen"] and length / width > p["lwTresh"]:
            accepted.append(hole)
    assert accepted == [1] and ref["n_boxes"] == 1 and ref["BOX"].any()
    monkeypatch.setenv("LFDMI_HOLE_PRUNE", "1")
    h, w = ref["frame"].shape
    with _native.Context(0, h, w, 1) as ctx:
        cnt = run_and_check(ctx, ref, "bright", name)
    assert int(cnt[hc.C_NHOLES]) == 2 and int(cnt[hc.C_NHOLES_PRUNED]) == 1 and int(cnt[fc.C_NQUADS]) == 1


def test_general_kernels_take_the_frame(oracle, monkeypatch):
    """LFDMI_FRAME_RUNCAP below the frame's runs: k_keys / k_extremes make every hole's key (no pruning there), same results."""
    from lfd_amd import _native
    name = "mixed_130x257"
    ref = reference(oracle, name, hc.FRAMES[name], "bright")
    h, w = ref["frame"].shape
    monkeypatch.setenv("LFDMI_HOLE_PRUNE", "1")
    monkeypatch.setenv("LFDMI_FRAME_RUNCAP", "8")
    with _native.Context(0, h, w, 1) as ctx:
        cnt = run_and_check(ctx, ref, "bright", name + " / LFDMI_FRAME_RUNCAP=8")
        assert ctx.stats()["general_reruns"] == 1
    assert int(cnt[hc.C_NHOLES]) == 0 and int(cnt[hc.C_NHOLES_PRUNED]) == 0


def test_hole_table_full(oracle, monkeypatch):
    """1 600 holes, more than the hole table's FRAME_HOLECAP entries, 800 of them roundish: those with a place in the table are
    measured and dropped, those without keep their keys and are looked up in the global tables."""
    from lfd_amd import _native
    ref = reference(oracle, "many", hc.f_many, "bright")
    assert ref["holes"] == 1600 > fc.FRAME_HOLECAP and ref["n_boxes"] == 1600
    h, w = ref["frame"].shape
    for prune in (0, 1):
        monkeypatch.setenv("LFDMI_HOLE_PRUNE", str(prune))
        with _native.Context(0, h, w, 1) as ctx:
            cnt = run_and_check(ctx, ref, "bright", f"many / LFDMI_HOLE_PRUNE={prune}")
            assert ctx.stats()["general_reruns"] == 0
        print("many: LFDMI_HOLE_PRUNE", prune, "counters (keys, slots, holes, pruned)", cnt[[0, 1, 20, 21]])
        assert int(cnt[hc.C_NHOLES]) == 1600
        if prune:
            # at most FRAME_HOLECAP holes have a place, so at least 576 have none: both kinds are among them (they alternate)
            assert 0 < int(cnt[hc.C_NHOLES_PRUNED]) < 800
            assert int(cnt[hc.C_NKEYS]) == 3200 - int(cnt[hc.C_NHOLES_PRUNED])
        else:
            assert int(cnt[hc.C_NHOLES_PRUNED]) == 0 and int(cnt[hc.C_NKEYS]) == 3200
