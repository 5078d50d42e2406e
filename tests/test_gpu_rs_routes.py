"""remove_stars on every route: each case of tests/rs_cases.py through lfdmi_remove_stars (per object and sorted) and through
lfdmi_detect_batch with its catalogue -- device, host, pinned and big-endian frames, a device catalogue with host frames, without
and with the 8-bit stage images, under every LFDMI_RS_* switch -- against the literal numpy slicing: the frame the caller gets
back bit for bit, every stage image the route leaves (the dim pass erodes 1 x 1, so ERODED shows the sweep's mask pixel by
pixel), the record and the count of accepted rectangles.  A failure names the case, the route, the stage, the number of
differing pixels and the first of them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import front_cases as fc
import rs_cases as R
from rs_cases import CASES, BY_NAME
from test_gpu_front_seams import check_record, stage_ids

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_KNOBS = ("LFDMI_RS_FOLD", "LFDMI_RS_SORT_MIN", "LFDMI_RS_FILL_AT", "LFDMI_RS_FILL_AT0", "LFDMI_RS_FILL_FRAC", "LFDMI_PREP_ROWS")
LOCS = ("device", "host", "pinned", "be", "devcat")
SWITCHES = ({"LFDMI_RS_FOLD": "0"}, {"LFDMI_RS_SORT_MIN": "0"}, {"LFDMI_RS_FILL_AT": "1"}, {"LFDMI_RS_FILL_AT": "3"}, {"LFDMI_RS_FILL_AT": "13"},
            {"LFDMI_RS_FILL_AT0": "-1"}, {"LFDMI_RS_FILL_AT0": "3"}, {"LFDMI_RS_SORT_MIN": "0", "LFDMI_RS_FOLD": "0"})
BATCH_CASES = [c for c in CASES if c.batch]
_refs = {}


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    for k in RS_KNOBS:
        monkeypatch.delenv(k, raising=False)


def set_knobs(monkeypatch, *dicts):
    for k in RS_KNOBS:
        monkeypatch.delenv(k, raising=False)
    merged = {}
    for d in dicts:
        merged.update(d)
    for k, v in merged.items():
        monkeypatch.setenv(k, v)
    return merged


def frame_ref(oracle, key, frame, cat, filter="r", rs=None, params=None):
    """literal's frame, the stage images of the dim pass on it and the oracle's record (computed once, shared, never written to)."""
    if key not in _refs:
        pb, pd = params or R.dim_params()
        lit = R.literal(frame, cat, filter, **(rs or {}))
        r = fc.reference(oracle, np.ascontiguousarray(lit[::-1]), pd, True)
        r["literal"] = lit
        if cat is None:
            r["record"] = oracle.detect_frame(np.array(frame), pb, pd)
        else:
            r["record"] = oracle.detect_frame(np.array(frame), pb, pd, cat, oracle.rs_params(filter, **dict(R.RS_DEFAULT, **(rs or {}))))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def case_ref(oracle, c):
    return frame_ref(oracle, c.name, c.frame, c.cat, c.filter, c.rs)


def rs_struct(c_or_filter="r", rs=None):
    from lfd_amd import _native
    if isinstance(c_or_filter, R.Case):
        return _native.make_rs_params(c_or_filter.filter, **c_or_filter.kw)
    return _native.make_rs_params(c_or_filter, **dict(R.RS_DEFAULT, **(rs or {})))


def pack(cats, device=False):
    from lfd_amd.catalogs import pack_catalogs
    p = pack_catalogs(cats)
    if device:
        import torch
        p = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in p.items()}
    return p


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def first_diff(got, want):
    bad = np.asarray(got) != np.asarray(want)
    idx = tuple(int(v) for v in np.argwhere(bad)[0])
    return f"{int(bad.sum())} pixels differ, first at {idx}: device {got[idx]!r}, reference {want[idx]!r}"


def run_batch(ctx, frames, loc, cats, rs, pb, pd):
    """One lfdmi_detect_batch on ``frames`` [n, h, w] (float32, the caller's orientation) -> (records, the frames the caller has
    afterwards as float32, the frames the caller may expect untouched: True for big-endian ones)."""
    import torch
    packed = pack(cats, device=loc == "devcat") if cats is not None else None
    if loc == "device":
        t = torch.from_numpy(np.array(frames)).cuda()
        rec = ctx.detect_batch(t, pb, pd, packed, rs)
        torch.cuda.synchronize()
        return rec, t.cpu().numpy(), False
    if loc == "pinned":
        buf, view = ctx.pinned_buffer(frames.nbytes), None
        try:
            view = buf.array[:frames.nbytes].view(np.float32).reshape(frames.shape)
            view[...] = frames
            rec = ctx.detect_batch(view, pb, pd, packed, rs, pinned=True)
            return rec, np.array(view), False
        finally:
            view = None
            buf.close()
    if loc == "be":
        a = np.ascontiguousarray(frames.astype(">f4"))
        rec = ctx.detect_batch(a, pb, pd, packed, rs)
        return rec, a.astype(np.float32), True
    a = np.array(frames)                                                    # "host", "devcat"
    rec = ctx.detect_batch(a, pb, pd, packed, rs)
    return rec, a, False


def check_images(ctx, slot, ref, fetch, shape, what):
    h, w = shape
    ids = stage_ids()
    quads = int(ctx.get_counters(slot, 1)[0, fc.C_NQUADS])
    assert quads == ref["n_boxes"], f"{what}: {quads} accepted rectangles on the device, {ref['n_boxes']} in the oracle"
    for st in fetch:
        got, want = ctx.get_stage(slot, ids[st], h, w), ref[st]
        if st in ("CANNY", "BOX"):
            got, want = got != 0, want != 0
        if not np.array_equal(got, want):
            pytest.fail(f"{what}: stage {st}: {first_diff(got, want)} (row, column in the flipped frame)")


def check_call(ctx, c_name, frames, cats, refs, loc, mode, knobs, pd, rec, back, untouched, slots=None, skip_images=()):
    n, h, w = frames.shape
    max_obj = max([0] + [len(c["NOBSERVE"]) for c in cats if c is not None]) if cats is not None else 0
    rt = R.route(h, w, max_obj, "device" if loc == "device" else "host", "device" if loc == "devcat" else "host", "be" if loc == "be" else "f32",
                 knobs, pd, mode)
    fetch = fc.route(h, w, pd, "batch", mode, knobs)["fetch"]
    for i in range(n):
        what = f"{c_name} / frame {i} of {n} / {loc} frames / stage images {mode} / knobs {knobs} / route {rt}"
        check_record(rec[i], refs[i]["record"], what)
        want = frames[i] if untouched else refs[i]["literal"]
        if not same_bits(back[i], want):
            pytest.fail(f"{what}: the frame the caller gets back: {first_diff(back[i], want)} (row, column)")
    assert slots is not None or n == 1
    for slot, i in ({0: 0} if slots is None else slots).items():
        if i not in skip_images:
            check_images(ctx, slot, refs[i], fetch, (h, w), f"{c_name} / frame {i} in slot {slot} / {loc} frames / stage images {mode} / knobs {knobs} / route {rt}")
    return rt


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_remove_stars_fill_in_front(oracle, monkeypatch, c):
    """lfdmi_remove_stars, per object (k_rs_fill) and sorted (k_rs_sort + k_rs_fill_bands), host and device frames: the literal
    slicing bit for bit, and a second call changes nothing.  LFDMI_RS_SORT_MIN is set both ways over the case's own knobs, so
    every case takes both routes where its shape allows the sort."""
    import torch
    from lfd_amd import _native
    for extra in ({"LFDMI_RS_SORT_MIN": str(R.RS_SORT_MIN)}, {"LFDMI_RS_SORT_MIN": "0"}):
        knobs = set_knobs(monkeypatch, c.knobs, extra)
        with _native.Context(0, c.h, c.w, 1) as ctx:
            for dev in (False, True):
                what = f"{c.name} / {'device' if dev else 'host'} frame / knobs {knobs}"
                img = torch.from_numpy(np.array(c.frame)).cuda() if dev else np.array(c.frame)
                for call in (1, 2):
                    ctx.remove_stars(img, pack([c.cat]), rs_struct(c))
                    got = img.cpu().numpy() if dev else img
                    if not same_bits(got, c.literal):
                        pytest.fail(f"{what} / call {call}: {first_diff(got, c.literal)} (row, column)")


@pytest.mark.parametrize("c", BATCH_CASES, ids=repr)
def test_detect_batch_with_the_catalogue(oracle, monkeypatch, c):
    from lfd_amd import _native
    pb, pd = R.dim_params()
    ref = case_ref(oracle, c)
    knobs = set_knobs(monkeypatch, c.knobs)
    for mode in (0, 1):
        for loc in LOCS:
            with _native.Context(0, c.h, c.w, 1) as ctx:
                ctx.set_stage_images(mode)
                rec, back, untouched = run_batch(ctx, c.frame[None], loc, [c.cat], rs_struct(c), pb, pd)
                rt = check_call(ctx, c.name, c.frame[None], [c.cat], [ref], loc, mode, knobs, pd, rec, back, untouched)
                assert ctx.stats()["spilled_frames"] == 0, (c, loc, mode, ctx.stats())
                if mode == 0 and loc == "device":
                    for k, v in c.expect.items():
                        assert rt[k] == v, (c, k, rt)


@pytest.mark.parametrize("c", BATCH_CASES, ids=repr)
def test_switches(oracle, monkeypatch, c):
    """Every LFDMI_RS_* switch on device frames (the side fill exists for them alone), fold and sort also on host frames: each
    result against the reference, so all of them equal the default's."""
    from lfd_amd import _native
    pb, pd = R.dim_params()
    ref = case_ref(oracle, c)
    for sw in SWITCHES:
        knobs = set_knobs(monkeypatch, c.knobs, sw)
        for loc in ("device", "host") if ("LFDMI_RS_FOLD" in sw or "LFDMI_RS_SORT_MIN" in sw) else ("device",):
            with _native.Context(0, c.h, c.w, 1) as ctx:
                ctx.set_stage_images(0)
                rec, back, untouched = run_batch(ctx, c.frame[None], loc, [c.cat], rs_struct(c), pb, pd)
                check_call(ctx, c.name, c.frame[None], [c.cat], [ref], loc, 0, knobs, pd, rec, back, untouched)
                assert ctx.stats()["spilled_frames"] == 0, (c, loc, knobs, ctx.stats())


def batch5(oracle):
    frames = np.stack([R.flat(40, 160)] * 5)
    cats = [R.batch_cat(n) for n in R.BATCH5]
    refs = [frame_ref(oracle, ("batch5", i), frames[i], cats[i]) for i in range(5)]
    return frames, cats, refs


@pytest.mark.parametrize("sort_min", (None, "0"))
def test_five_frames_five_catalogues_two_slots(oracle, monkeypatch, sort_min):
    """cat_f0 + c0: chunks of 2 + 2 + 1 frames, each with its own catalogue row (counts 5, 0, 1, 8, 5 under a max_obj of 8); the
    first four alone, so that the second chunk's slots are fetched too (the single object beside eight); then the five again
    after a call with a larger max_obj and after one with a smaller: squares beyond ``count`` and squares of the earlier call
    are never applied."""
    from lfd_amd import _native
    pb, pd = R.dim_params()
    frames, cats, refs = batch5(oracle)
    big = [R.catalogue(R.BATCH_BIGGER)] * 2
    small = [R.catalogue(R.BATCH_SMALLER)]
    ref_big = frame_ref(oracle, "batch_bigger", frames[0], big[0])
    ref_small = frame_ref(oracle, "batch_smaller", frames[0], small[0])
    knobs = set_knobs(monkeypatch, {} if sort_min is None else {"LFDMI_RS_SORT_MIN": sort_min})
    for mode in (0, 1):
        for loc in ("device", "host", "be", "devcat"):
            with _native.Context(0, 40, 160, 2) as ctx:
                ctx.set_stage_images(mode)
                for step in ("five", "four", "bigger", "five", "smaller", "five"):
                    if step == "four":
                        rec, back, untouched = run_batch(ctx, frames[:4], loc, cats[:4], rs_struct(), pb, pd)
                        check_call(ctx, "batch5, its first four", frames[:4], cats[:4], refs[:4], loc, mode, knobs, pd, rec, back, untouched, slots={0: 2, 1: 3})
                    elif step == "five":
                        rec, back, untouched = run_batch(ctx, frames, loc, cats, rs_struct(), pb, pd)
                        check_call(ctx, "batch5 after " + step, frames, cats, refs, loc, mode, knobs, pd, rec, back, untouched, slots={0: 4})
                    elif step == "bigger":
                        rec, back, untouched = run_batch(ctx, frames[:2], loc, big, rs_struct(), pb, pd)
                        check_call(ctx, "bigger", frames[:2], big, [ref_big] * 2, loc, mode, knobs, pd, rec, back, untouched, slots={0: 0, 1: 1})
                    else:
                        rec, back, untouched = run_batch(ctx, frames[:1], loc, small, rs_struct(), pb, pd)
                        check_call(ctx, "smaller", frames[:1], small, [ref_small], loc, mode, knobs, pd, rec, back, untouched, slots={0: 0})
                assert ctx.stats()["spilled_frames"] == 0


def test_eight_slots_two_of_them_decided_by_the_bright_pass(oracle):
    """The bright pass (its usual lwTresh) decides the two streak frames, so the dim pass works on six of the eight slots while the
    second part of the side fill runs: every frame comes back blotted, the six undecided ones leave the dim pass's images."""
    from lfd_amd import _native
    pb, pd = fc.default_params()
    pd = dict(pd, erodeKernel=R.ERODE_1x1)
    pairs = R.batch8()
    frames = np.stack([f for f, _ in pairs])
    cats = [cat for _, cat in pairs]
    refs = [frame_ref(oracle, ("batch8", i), frames[i], cats[i], params=(pb, pd)) for i in range(8)]
    decided = [i for i, n in enumerate(R.BATCH8) if n == "STREAK"]
    assert [r["record"]["found"] for r in refs] == [1 if i in decided else 0 for i in range(8)]
    for mode in (0, 1):
        for loc in ("device", "host"):
            with _native.Context(0, *R.BATCH8_SHAPE, 8) as ctx:
                ctx.set_stage_images(mode)
                rec, back, untouched = run_batch(ctx, frames, loc, cats, rs_struct(), pb, pd)
                check_call(ctx, "batch8", frames, cats, refs, loc, mode, {}, pd, rec, back, untouched, slots={i: i for i in range(8)}, skip_images=decided)
                assert ctx.stats()["spilled_frames"] == 0, (loc, mode, ctx.stats())


def test_overflowing_frames_run_again_alone_with_their_catalogue_row(oracle, monkeypatch):
    """Tiny tables that may not grow (LFDMI_GROW=0): the crowded frames overflow them and are run again, alone, in the worst-case workspace.  Big-endian frames are
    never blotted in place, so the rerun needs the frame's own catalogue row (cat_f0 + c0 + i); device and host frames were
    blotted by the first run."""
    from lfd_amd import _native
    monkeypatch.setenv("LFDMI_GROW", "0")
    pb, pd = R.dim_params()
    cs = [BY_NAME[n] for n in R.SPILL_CASES]
    frames = np.stack([c.frame for c in cs])
    cats = [c.cat for c in cs]
    refs = [case_ref(oracle, c) for c in cs]
    for loc in ("be", "device", "host"):
        with _native.Context(0, cs[0].h, cs[0].w, 2, caps=R.SPILL_CAPS) as ctx:
            ctx.set_stage_images(0)
            rec, back, untouched = run_batch(ctx, frames, loc, cats, rs_struct(), pb, pd)
            check_call(ctx, "spill", frames, cats, refs, loc, 0, {}, pd, rec, back, untouched, slots={})
            assert ctx.stats()["spilled_frames"] >= 2, (loc, ctx.stats())


@pytest.mark.parametrize("env", R.CHILD_ENVS, ids=lambda e: "_".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_knobs_read_once_per_process(oracle, tmp_path, env):
    """LFDMI_PREP_ROWS (the rows of a sweep workgroup, so of its LDS mask) and LFDMI_RS_FILL_FRAC (the first part's share of the
    side fill) are read once per process: a fresh child interpreter runs four cases against the references saved here."""
    data = {}
    for name in R.CHILD_CASES:
        ref = case_ref(oracle, BY_NAME[name])
        for k in ("ERODED", "CANNY", "BOX", "literal"):
            data[f"{k}_{name}"] = ref[k]
        data[f"record_{name}"] = np.array(json.dumps(ref["record"]))
        data[f"nboxes_{name}"] = np.int64(ref["n_boxes"])
    npz = tmp_path / "rs_ref.npz"
    np.savez(npz, **data)
    child_env = {k: v for k, v in os.environ.items() if k not in RS_KNOBS}
    child_env.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rs_child.py"), str(npz)], env=child_env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert [line.split()[0] for line in r.stdout.splitlines() if line.endswith(" ok")] == sorted(R.CHILD_CASES)
