"""The measurement units where a call splits: chunks of jobs, staging slots, batches of cells, persistent blocks on a second list
item, chunks of frames (source finder) and groups of frames and launches (stacked cross-sections).  The sizes that decide the
split are compiled in (8 Mi pairs, 512 MiB, 2048 blocks ...) and no quick input reaches them, so every test lowers them on a
context of its own with ``Context.debug_unit_limits`` and reads the split back with ``Context.debug_unit_split``: the expected
split is worked out here from the rule include/lfdmi.h documents, never taken from the library, and (but where the rule says a
limit has no effect) differs from the unsplit one, so a limit that a unit ignored would fail the readback.  Every result is
compared bit for bit with the unit's numpy restatement, which knows nothing of chunks: no tolerance appears.

Inputs: 37 x 130 (partial tiles on both axes, w % 4 != 0) and 48 x 256 (whole tiles, the vector loads); nine frames of which
0, 1, 3, 4, 6 and 8 carry segments (six jobs with gaps), frame 3 about 140 short ones (more than an LDS chunk of 128), the others
2 to 6 with BAD and TOO_LONG ones among them, interleaved."""
import contextlib
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as IR  # noqa: E402
import lc_ref as LR  # noqa: E402
import mask_ref as MR  # noqa: E402
import stack_ref as S  # noqa: E402
import stars_ref as R  # noqa: E402
import strip_ref as SR  # noqa: E402
import sub_ref as UR  # noqa: E402
import test_gpu_inject as TI  # noqa: E402
import test_gpu_lc as TL  # noqa: E402
import test_gpu_masks as TM  # noqa: E402
import test_gpu_stack as TK  # noqa: E402
import test_gpu_strips as TS  # noqa: E402
import test_gpu_sub as TU  # noqa: E402
from test_gpu_lc import plane, special_frames  # noqa: E402
from test_gpu_stars import assert_records  # noqa: E402
from test_gpu_stars_tiles import blob  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(37, 130), (48, 256)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
N_FRAMES = 9
CARRY = (0, 1, 3, 4, 6, 8)    # the frames that carry segments; 2, 5 and 7 carry none
BIG = 3                       # ... about 140 short ones
MAX_SEC = 64
SKIP = 0x05
LOCS = ("host", "pinned", "device")
# the compiled defaults (include/lfdmi.h: lfdmi_debug_unit_limits)
LIST_PAIRS, STAGE_BYTES, RENDER_BLOCKS = 8 << 20, 512 << 20, 2048


def ceil_div(a, b):
    return -(-a // b)


def tiles(shape):
    return ceil_div(shape[1], 64) * ceil_div(shape[0], 16)


def settings(shape, plane_only=False):
    """name -> limits.  ``plane_only``: the call stages a byte per pixel and no frame (mask_trails without a fill)"""
    nt, N = tiles(shape), shape[0] * shape[1]
    return {
        "pairs-1job": dict(list_pairs=nt),                 # CH = 1: six chunks, every job in staging slot 0
        "pairs-2jobs": dict(list_pairs=2 * nt + 1),        # CH = 2: 2, 2, 2
        "pairs-4jobs": dict(list_pairs=4 * nt),            # CH = 4: 4 + 2, a ragged last chunk that reuses slots 0 and 1
        "stage-2jobs": dict(stage_bytes=2 * N if plane_only else 2 * (4 * N + N)),   # two frames and two planes
        "stage-1byte": dict(stage_bytes=1),                # clamps to one job per chunk
        "blocks-1": dict(render_blocks=1),                 # one block walks every item
        "blocks-3": dict(render_blocks=3),                 # three blocks take items of different jobs in turn
    }


SETTINGS = list(settings(SHAPES[0]))


def jobs_per_chunk(shape, lim, job_bytes):
    """the documented rule: max(1, list_pairs / tiles) jobs, and max(1, stage_bytes / staged bytes of a job) where a job stages any"""
    ch = max(1, min(lim.get("list_pairs", LIST_PAIRS), LIST_PAIRS) // tiles(shape))
    if job_bytes:
        ch = min(ch, max(1, min(lim.get("stage_bytes", STAGE_BYTES), STAGE_BYTES) // job_bytes))
    return ch


def expect_split(shape, lim, job_bytes, jobs):
    """(chunks, grid) of a call of ``jobs`` jobs in one row"""
    ch = jobs_per_chunk(shape, lim, job_bytes)
    return ceil_div(jobs, ch), min(min(ch, jobs) * tiles(shape), min(lim.get("render_blocks", RENDER_BLOCKS), RENDER_BLOCKS))


def check_split(ctx, what, shape, lim, job_bytes, jobs):
    got = ctx.debug_unit_split()
    want = expect_split(shape, lim, job_bytes, jobs)
    print(what, lim, got)
    assert (got["chunks"], got["grid"]) == want, (what, lim, got, want)
    unsplit = (1, jobs * tiles(shape))
    if set(lim) == {"stage_bytes"} and not job_bytes:
        assert want == unsplit, what                                      # nothing is staged: the limit has no effect
    else:
        assert want != unsplit, (what, lim, want)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


@contextlib.contextmanager
def located(ctx, loc, frames, mask=None, be=False):
    """``frames`` (and a plane) where ``loc`` says, as copies -> (frames, plane, the binding's keyword for pinned memory).  Pinned
    frames are big-endian with ``be``; the views die with the block."""
    if loc == "host":
        yield frames.copy(), None if mask is None else mask.copy(), {}
    elif loc == "device":
        import torch
        yield torch.from_numpy(frames.copy()).cuda(), None if mask is None else torch.from_numpy(mask.copy()).cuda(), {}
    else:
        fb = ctx.pinned_buffer(frames.nbytes)
        mb = ctx.pinned_buffer(mask.nbytes if mask is not None else 1)
        pf = fb.array.view(">f4" if be else "<f4")[:frames.size].reshape(frames.shape)
        pf[...] = frames
        pm = None
        if mask is not None:
            pm = mb.array.view(np.uint8)[:mask.size].reshape(mask.shape)
            pm[...] = mask
        try:
            yield pf, pm, dict(pinned=True)
        finally:
            del pf, pm
            fb.close()
            mb.close()


def open_ctx():
    from lfd_amd import _native
    return _native.Context(0, 48, 256, 2)


def spread(random_segments, shape, seed, extra):
    """the segments of a case: frame 3 gets 140 short ones, the other carrying frames 2 to 6, ``extra`` (BAD and TOO_LONG ones)
    among them; interleaved (the library sorts them by frame)"""
    out = list(extra)
    for f in CARRY:
        out += random_segments(shape, f, 140, seed + f, short=True) if f == BIG else random_segments(shape, f, 2 + f % 5, seed + f)
    return out


def interleave(segs, dtype):
    segs = np.array(segs, dtype)
    return segs[np.random.default_rng(7).permutation(len(segs))]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def job_frames(segs, good):
    """the frames that carry a good segment, ascending: the jobs"""
    return sorted({int(f) for f in segs["frame"][good]})


# ---- light curves -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lc_case(shape):
    extra = [LR.segment(1, np.nan, 3.0, 9.0, 3.0), LR.segment(6, 3.0, 3.0, 3.0, 3.0), LR.segment(4, -1000.0, 5.0, 1000.0, 6.0, half=2.0)]
    segs = interleave(spread(TL.random_segments, shape, 900, extra), LR.SEGMENT_DTYPE)
    frames, m = special_frames(shape, 5, n=N_FRAMES), plane(shape, 11, n=N_FRAMES)
    kw = dict(max_sections=MAX_SEC, **TL.PARAMS)
    want, want_m = LR.light_curves(frames, segs, **kw), LR.light_curves(frames, segs, mask=m, skip_bits=SKIP, **kw)
    assert {LR.BAD_SEGMENT, LR.TOO_LONG, LR.OK} <= set(want[0]["status"].tolist())
    jobs = job_frames(segs, np.isin(want[0]["status"], (LR.OK, LR.EMPTY)))
    assert jobs == list(CARRY)
    frozen(segs, frames, m, *want, *want_m)
    return segs, frames, m, want, want_m


def lc_equal(what, got, want):
    TL.assert_same(what + " sections", got[1], want[1])
    TL.assert_same(what + " records", got[0], want[0])


@pytest.mark.parametrize("name", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_light_curves_in_chunks(shape, name):
    segs, frames, m, want, want_m = lc_case(shape)
    lim, N = settings(shape)[name], shape[0] * shape[1]
    kw = dict(max_sections=MAX_SEC, **TL.PARAMS)
    with open_ctx() as ctx:
        for loc in LOCS:
            for mask, w in ((None, want), (m, want_m)):
                what = f"light_curves {loc} {'masked' if mask is not None else 'plain'}"
                with located(ctx, loc, frames, mask, be=True) as (f, pm, pin):
                    mk = dict(mask=pm, skip_bits=SKIP) if mask is not None else {}
                    ctx.debug_unit_limits()
                    lc_equal(what + " no limits", ctx.light_curves(f, segs, **mk, **pin, **kw), w)
                    assert ctx.debug_unit_split()["chunks"] == 1 and ctx.debug_unit_split()["grid"] == len(CARRY) * tiles(shape)
                    ctx.debug_unit_limits(**lim)
                    lc_equal(what, ctx.light_curves(f, segs, **mk, **pin, **kw), w)
                check_split(ctx, what, shape, lim, 0 if loc == "device" else 4 * N + (N if mask is not None else 0), len(CARRY))


# ---- trail masks ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case(shape):
    extra = [MR.segment(1, np.nan, 3.0, 9.0, 3.0, half=2.0, bits=1), MR.segment(6, 3.0, 3.0, 3.0, 3.0, half=2.0, bits=1)]
    segs = interleave(spread(TM.random_segments, shape, 700, extra), MR.SEGMENT_DTYPE)
    frames = special_frames(shape, 6, n=N_FRAMES)
    filled = frames.copy()
    mask, stats, counts = MR.mask_trails(segs, (N_FRAMES, *shape), frames=filled, fill="value")
    assert job_frames(segs, stats["status"] != MR.BAD_SEGMENT) == list(CARRY) and MR.BAD_SEGMENT in stats["status"]
    assert not np.array_equal(TM.u32(filled), TM.u32(frames))
    for f in (2, 5, 7):
        assert np.array_equal(TM.u32(filled[f]), TM.u32(frames[f])) and not mask[f].any()
    frozen(segs, frames, filled, mask, stats, counts)
    return segs, frames, filled, mask, stats, counts


# (frames, plane): where each is; None: no frames, no fill.  f_stage and m_stage of mask.hip are independent
MASK_ROUTES = [("host", "host"), ("host", "device"), ("device", "host"), (None, "host"), ("device", "device"), ("pinned", "pinned")]


@pytest.mark.parametrize("name", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mask_trails_in_chunks(shape, name):
    import torch
    segs, frames, filled, want_mask, want_stats, want_counts = mask_case(shape)
    N = shape[0] * shape[1]
    with open_ctx() as ctx:
        for floc, mloc in MASK_ROUTES:
            what = f"mask_trails frames {floc} plane {mloc}"
            f_stage, m_stage = floc in ("host", "pinned"), mloc in ("host", "pinned")
            lim = settings(shape, plane_only=m_stage and not f_stage)[name]
            # what the plane holds before each call: 0xEE for a clearing call (nothing of it may stay), random bytes for an ORing
            # one (all of it stays, under the new bits: the plane of a later chunk's job is staged in before it is ORed onto)
            before = {True: np.full((N_FRAMES, *shape), 0xEE, np.uint8),
                      False: np.random.default_rng(8).integers(0, 256, (N_FRAMES, *shape)).astype(np.uint8)}
            with located(ctx, floc or "host", frames, before[True] if mloc == floc else None) as (f, pm, pin):
                if mloc != floc:
                    pm = torch.from_numpy(before[True].copy()).cuda() if mloc == "device" else before[True].copy()
                for clear in (True, False):
                    want_plane = want_mask if clear else want_mask | before[False]
                    assert clear or not np.array_equal(want_plane, want_mask)
                    for limits in ({}, lim):
                        # frames and plane are as new before every call: no call may live off what the one before it left
                        if floc is not None:
                            f[...] = torch.from_numpy(frames.copy()).cuda() if floc == "device" else frames
                        pm[...] = torch.from_numpy(before[clear].copy()).cuda() if mloc == "device" else before[clear]
                        ctx.debug_unit_limits(**limits)
                        if floc is None:
                            _, stats, counts = ctx.mask_trails(None, segs, mask=pm, clear=clear)
                        else:
                            _, stats, counts = ctx.mask_trails(f, segs, mask=pm, fill="value", clear=clear, **pin)
                            TM.assert_equal(what + " frames", TM.u32(host(f)), TM.u32(filled))
                        TM.assert_equal(what + f" mask clear={clear}", host(pm), want_plane)
                        TM.assert_equal(what + " n_pix", stats["n_pix"], want_stats["n_pix"])
                        TM.assert_equal(what + " status", stats["status"], want_stats["status"])
                        TM.assert_equal(what + " frame_counts", counts, want_counts)
                        if not limits:
                            assert ctx.debug_unit_split()["chunks"] == 1
                    check_split(ctx, what + f" clear={clear}", shape, lim, (4 * N if f_stage else 0) + (N if m_stage else 0), len(CARRY))


# ---- trail injection --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inject_case(shape):
    h, w = shape
    rng = np.random.default_rng(41)
    tr = []
    for f in CARRY:
        for _ in range(140 if f == BIG else 2 + f % 5):
            theta = float(rng.uniform(0.0, math.pi))
            x, y = float(rng.uniform(0, w)), float(rng.uniform(0, h))
            tm = TI.along(x, y, theta)
            ends = dict(t0=tm - float(rng.uniform(2, 12)), t1=tm + float(rng.uniform(2, 12))) if f == BIG or rng.random() < 0.5 else {}
            tr.append(IR.trail(f, int(rng.integers(0, 2)), TI.through(shape, x, y, theta), theta, amplitude=float(rng.uniform(-1, 2)), **ends))
    tr = interleave(tr, IR.TRAIL_DTYPE)
    tabs, step = TI.tables()
    frames = special_frames(shape, 8, n=N_FRAMES)
    want = IR.inject(frames.copy(), tr, tabs, step, 2)
    for f in (2, 5, 7):
        assert np.array_equal(TI.bits(want[f]), TI.bits(frames[f]))
    assert all(not np.array_equal(TI.bits(want[f]), TI.bits(frames[f])) for f in CARRY)
    frozen(tr, frames, want)
    return tr, tabs, step, frames, want


@pytest.mark.parametrize("name", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_inject_trails_in_chunks(shape, name):
    tr, tabs, step, frames, want = inject_case(shape)
    lim, N = settings(shape)[name], shape[0] * shape[1]
    with open_ctx() as ctx:
        for loc in LOCS:
            what = f"inject_trails {loc}"
            for limits in ({}, lim):
                with located(ctx, loc, frames) as (f, _, pin):
                    ctx.debug_unit_limits(**limits)
                    ctx.inject_trails(f, tr, tabs, step, subsample=2, **pin)
                    TI.assert_same_bits(host(f), want)
                if not limits:
                    assert ctx.debug_unit_split()["chunks"] == 1
            check_split(ctx, what, shape, lim, 0 if loc == "device" else 4 * N, len(CARRY))


# ---- trail strips -----------------------------------------------------------------------------------------------------------------
def strip_segments(shape):
    extra = [SR.segment(1, np.nan, 3.0, 9.0, 3.0), SR.segment(6, 3.0, 3.0, 3.0, 3.0), SR.segment(4, -1000.0, 5.0, 1000.0, 6.0, half=2.0),
             SR.segment(0, 1.0, 3.0, 9.0, 3.0, half=64.6)]
    return interleave(spread(TS.random_segments, shape, 500, extra), SR.SEGMENT_DTYPE)


def sorted_cells(segs, rec, good_status):
    """(frame, cells) of every good segment in the library's order: by frame, ascending index within a frame"""
    good = np.nonzero(np.isin(rec["status"], good_status))[0]
    order = good[np.argsort(segs["frame"][good], kind="stable")]
    return [(int(segs["frame"][i]), int(rec["n_sec"][i]) * int(rec["n_off"][i])) for i in order]


@functools.lru_cache(maxsize=None)
def strip_case(shape):
    segs = strip_segments(shape)
    frames, m = special_frames(shape, 5, n=N_FRAMES), plane(shape, 11, n=N_FRAMES)
    kw = dict(max_sections=MAX_SEC, **TS.PARAMS)
    want = SR.trail_strips(frames, segs, **kw)
    want_m = SR.trail_strips(frames, segs, mask=m, skip_bits=SKIP, max_cells=want[2].shape[1], **kw)
    assert {SR.BAD_SEGMENT, SR.TOO_LONG, SR.OK} <= set(want[0]["status"].tolist())
    cells = sorted_cells(segs, want[0], (SR.OK, SR.EMPTY))
    assert sorted({f for f, _ in cells}) == list(CARRY) and sum(1 for f, _ in cells if f == BIG) == 140
    frozen(segs, frames, m, *want, *want_m)
    return segs, frames, m, want, want_m, cells


def strip_batches(cells, cell_bytes):
    """the greedy rule: a new batch when the next segment's cells no longer fit; a batch's first segment always does -> the
    batches as lists of (frame, cells)"""
    cap, out, inside = cell_bytes // 16, [[]], 0
    for f, c in cells:
        if inside > 0 and inside + c > cap:
            out.append([])
            inside = 0
        out[-1].append((f, c))
        inside += c
    return out


def expect_strip_split(shape, lim, job_bytes, cells):
    """(chunks, batches, grid): every batch's jobs (its frames; a frame two batches share is a job of both) go in chunks"""
    batches = strip_batches(cells, lim["cell_bytes"]) if "cell_bytes" in lim else [cells]
    ch = jobs_per_chunk(shape, lim, job_bytes)
    jobs = [len({f for f, _ in b}) for b in batches]
    grid = min(min(ch, max(jobs)) * tiles(shape), lim.get("render_blocks", RENDER_BLOCKS))
    return sum(ceil_div(j, ch) for j in jobs), len(batches), grid


def run_strips(ctx, shape, lim, what, locs=LOCS):
    segs, frames, m, want, want_m, cells = strip_case(shape)
    N = shape[0] * shape[1]
    kw = dict(max_sections=MAX_SEC, max_cells=want[2].shape[1], **TS.PARAMS)
    for loc in locs:
        for mask, w in ((None, want), (m, want_m)):
            tag = f"{what} {loc} {'masked' if mask is not None else 'plain'}"
            with located(ctx, loc, frames, mask, be=True) as (f, pm, pin):
                mk = dict(mask=pm, skip_bits=SKIP) if mask is not None else {}
                ctx.debug_unit_limits()
                TS.assert_all(tag + " no limits", ctx.trail_strips(f, segs, **mk, **pin, **kw), w)
                assert ctx.debug_unit_split() == dict(chunks=1, batches=1, grid=len(CARRY) * tiles(shape), launches=0)
                ctx.debug_unit_limits(**lim)
                TS.assert_all(tag, ctx.trail_strips(f, segs, **mk, **pin, **kw), w)
            got = ctx.debug_unit_split()
            exp = expect_strip_split(shape, lim, 0 if loc == "device" else 4 * N + (N if mask is not None else 0), cells)
            print(tag, lim, got)
            assert (got["chunks"], got["batches"], got["grid"]) == exp, (tag, lim, got, exp)
            if set(lim) == {"stage_bytes"} and loc == "device":
                assert exp == (1, 1, len(CARRY) * tiles(shape))
            else:
                assert exp != (1, 1, len(CARRY) * tiles(shape)), (tag, exp)


@pytest.mark.parametrize("name", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_trail_strips_in_chunks(shape, name):
    with open_ctx() as ctx:
        run_strips(ctx, shape, settings(shape)[name], "trail_strips")


def strip_cell_settings(shape):
    cells = strip_case(shape)[5]
    big = [c for f, c in cells if f == BIG]
    third = 16 * (sum(c for _, c in cells) // 3)
    return {
        "segment-per-batch": dict(cell_bytes=16),                               # every segment is its own batch
        "half-of-frame-3": dict(cell_bytes=16 * (sum(big[:70]) + 1)),           # the 140-segment frame is a job of two batches
        "thirds": dict(cell_bytes=third),                                       # batches that begin mid-frame and mid-chunk
        "thirds-1job": dict(cell_bytes=third, list_pairs=tiles(shape)),
        "thirds-1block": dict(cell_bytes=third, render_blocks=1),
    }


@pytest.mark.parametrize("name", ["segment-per-batch", "half-of-frame-3", "thirds", "thirds-1job", "thirds-1block"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_trail_strips_in_batches_of_cells(shape, name):
    lim = strip_cell_settings(shape)[name]
    cells = strip_case(shape)[5]
    batches = strip_batches(cells, lim["cell_bytes"])
    if name == "segment-per-batch":
        assert len(batches) == len(cells)
    else:
        shared = [sum(1 for b in batches if any(f == fr for f, _ in b)) for fr in CARRY]
        assert len(batches) >= 3 and max(shared) >= 2 and shared[CARRY.index(BIG)] >= 2      # a frame that is a job of two batches
        assert any(b[0][0] == a[-1][0] for a, b in zip(batches, batches[1:]))               # a batch that begins mid-frame
    with open_ctx() as ctx:
        run_strips(ctx, shape, lim, "trail_strips " + name)


def test_summed_over_offsets_a_strip_is_a_light_curve_with_both_units_split():
    """``trail_strips`` cells summed over b are ``light_curves``' n_geom, n_core and q_core at sec_len 8, the strips in batches of
    a third of the cells and chunks of one job, the light curves in chunks of two jobs walked by three blocks"""
    shape = (37, 130)
    segs, frames, m, _, _, cells = strip_case(shape)
    lsegs = np.zeros(len(segs), LR.SEGMENT_DTYPE)
    for k in ("frame", "x1", "y1", "x2", "y2", "half"):
        lsegs[k] = segs[k]
    lsegs["bg_in"], lsegs["bg_out"] = segs["half"] + 1.0, segs["half"] + 3.0
    N = shape[0] * shape[1]
    with open_ctx() as ctx:
        for kw in ({}, dict(mask=m, skip_bits=0x22)):
            ctx.debug_unit_limits(**strip_cell_settings(shape)["thirds-1job"])
            rec, sec, cel = ctx.trail_strips(frames, segs, max_sections=MAX_SEC, sec_len=8.0, **kw)
            assert ctx.debug_unit_split()["batches"] >= 3
            ctx.debug_unit_limits(stage_bytes=2 * 5 * N, render_blocks=3)
            lrec, lsec = ctx.light_curves(frames, lsegs, max_sections=MAX_SEC, sec_len=8.0, **kw)
            assert (ctx.debug_unit_split()["chunks"], ctx.debug_unit_split()["grid"]) == (3, 3)
            checked = 0
            for i in range(len(segs)):
                if rec[i]["status"] not in (SR.OK, SR.EMPTY):
                    continue
                assert lrec[i]["status"] in (LR.OK, LR.EMPTY) and lrec[i]["n_sec"] == rec[i]["n_sec"], i
                ns, no = int(rec[i]["n_sec"]), int(rec[i]["n_off"])
                c = cel[i][:ns * no].reshape(ns, no)
                assert np.array_equal(c["n_geom"].sum(1), lsec[i, :ns]["n_geom"]), i
                assert np.array_equal(c["n"].sum(1), lsec[i, :ns]["n_core"]), i
                assert np.array_equal(c["q"].sum(1), lsec[i, :ns]["q_core"]), i
                checked += int(c["n_geom"].sum() > 0)
            assert checked > 20


# ---- trail subtraction ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sub_case(shape):
    segs = strip_segments(shape)
    frames, m = special_frames(shape, 5, n=N_FRAMES), plane(shape, 11, n=N_FRAMES)
    kw = dict(max_sections=MAX_SEC, **TU.PARAMS)
    want = UR.subtract_trails(frames, segs, **kw)
    want_m = UR.subtract_trails(frames, segs, mask=m, skip_bits=SKIP, max_cells=want[2].shape[1], **kw)
    rec = want[1]
    assert {UR.BAD_SEGMENT, UR.TOO_LONG, UR.OK} <= set(rec["status"].tolist())
    cells = sorted_cells(segs, rec, (UR.OK, UR.EMPTY))
    per_frame = [sum(c for f, c in cells if f == fr) for fr in CARRY]
    assert all(per_frame)
    for f in CARRY:                                                           # every chunk has a frame that changes and a model
        on = (segs["frame"] == f) & (rec["status"] == UR.OK)
        assert int(rec["n_pix"][on].sum()) > 0 and not np.array_equal(TM.u32(want[0][f]), TM.u32(frames[f]))
    for f in (2, 5, 7):
        assert np.array_equal(TM.u32(want[0][f]), TM.u32(frames[f]))
    frozen(segs, frames, m, *want, *want_m)
    return segs, frames, m, want, want_m, per_frame


def expect_sub_split(shape, lim, job_bytes, per_frame):
    """(chunks, grid): a new chunk after CH jobs, or when the next frame's cells no longer fit (a chunk's first frame always does)"""
    ch = jobs_per_chunk(shape, lim, job_bytes)
    cap = min(lim.get("cell_bytes", 512 << 20), 512 << 20) // 16
    chunks, jobs_in, inside = [0], 0, 0
    for c in per_frame:
        if jobs_in > 0 and (jobs_in >= ch or inside + c > cap):
            chunks.append(0)
            jobs_in, inside = 0, 0
        chunks[-1] += 1
        jobs_in += 1
        inside += c
    return len(chunks), min(max(chunks) * tiles(shape), lim.get("render_blocks", RENDER_BLOCKS))


def run_sub(ctx, shape, lim, what, locs=LOCS, applies=(1, 0), models=(True,)):
    segs, frames, m, want, want_m, per_frame = sub_case(shape)
    N = shape[0] * shape[1]
    kw = dict(max_sections=MAX_SEC, max_cells=want[2].shape[1], **TU.PARAMS)
    for loc in locs:
        for mask, w in ((None, want), (m, want_m)):
            for apply in applies:
                for model in models:
                    tag = f"{what} {loc} {'masked' if mask is not None else 'plain'} apply={apply} model={model}"
                    for limits in ({}, lim):
                        # (apply = 1 changes native frames only: pinned frames are big-endian where nothing is written)
                        with located(ctx, loc, frames, mask, be=not apply) as (f, pm, pin):
                            mk = dict(mask=pm, skip_bits=SKIP) if mask is not None else {}
                            ctx.debug_unit_limits(**limits)
                            rec, tab = ctx.subtract_trails(f, segs, want_model=model, apply=apply, **mk, **pin, **kw)
                            # every frame of every chunk, not only the last; the frames that carry nothing among them
                            TU.same_bits(tag + " frames", host(f).astype(np.float32), w[0] if apply else frames)
                        TU.assert_same(tag + " records", rec, w[1])
                        if model:
                            TU.same_bits(tag + " model", tab, w[2])
                        else:
                            assert tab is None
                        if not limits:
                            assert ctx.debug_unit_split()["chunks"] == 1
                    got = ctx.debug_unit_split()
                    exp = expect_sub_split(shape, lim, 0 if loc == "device" else 4 * N + (N if mask is not None else 0), per_frame)
                    print(tag, lim, got)
                    assert (got["chunks"], got["grid"]) == exp, (tag, lim, got, exp)
                    if set(lim) == {"stage_bytes"} and loc == "device":
                        assert exp == (1, len(CARRY) * tiles(shape))
                    else:
                        assert exp != (1, len(CARRY) * tiles(shape)), (tag, exp)


@pytest.mark.parametrize("name", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_subtract_trails_in_chunks(shape, name):
    with open_ctx() as ctx:
        run_sub(ctx, shape, settings(shape)[name], "subtract_trails")


@pytest.mark.parametrize("name", ["frame-per-chunk", "two-small-frames"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_subtract_trails_in_chunks_of_cells(shape, name):
    per_frame = sub_case(shape)[5]
    small = sorted(c for f, c in zip(CARRY, per_frame) if f != BIG)
    # 16 bytes: a single frame exceeds the cap and is a chunk of its own; or the cells of the two largest of the small frames
    lim = dict(cell_bytes=16) if name == "frame-per-chunk" else dict(cell_bytes=16 * (small[-1] + small[-2]))
    chunks = expect_sub_split(shape, lim, 0, per_frame)[0]
    assert chunks == len(CARRY) if name == "frame-per-chunk" else 2 <= chunks < len(CARRY)
    with open_ctx() as ctx:
        run_sub(ctx, shape, lim, "subtract_trails " + name, models=(True, False))


# ---- source finder ----------------------------------------------------------------------------------------------------------------
STARS_SHAPE = (48, 256)
STARS_OBJ = 16


@functools.lru_cache(maxsize=None)
def stars_case():
    """six frames, each with its own stars on and beside the corners of the 64 x 16 tiles, and its own sigma"""
    h, w = STARS_SHAPE
    rng = np.random.default_rng(48256)
    frames = rng.normal(0, 0.025, (6, h, w)).astype(np.float32)
    xs, ys = (0, 63, 64, 65, 127, 128, 191, 192, w - 1), (0, 15, 16, 17, 31, 32, h - 1)
    for f in range(6):
        for k in range(3 + f):
            blob(frames[f], ys[(2 * k + f) % len(ys)], xs[(3 * k + 2 * f) % len(xs)], 2.0 + k + 0.5 * f, half=2)
    sigma = np.linspace(0.02, 0.045, 6).astype(np.float32)
    want = R.find_stars_batch(frames, sigma, max_obj=STARS_OBJ)
    assert len(set(want[1]["n_out"].tolist())) > 2 and want[1]["n_out"].min() >= 2
    frozen(frames, sigma, *want)
    return frames, sigma, want


@pytest.mark.parametrize("name", ["stage-1frame", "stage-2frames", "records-1frame", "records-2frames", "records-2-stage-1"])
def test_find_stars_in_chunks_of_frames(name):
    from lfd_amd import _native
    frames, sigma, want = stars_case()
    FB, RB = frames[0].nbytes, STARS_OBJ * 32
    lim = {"stage-1frame": dict(stage_bytes=FB), "stage-2frames": dict(stage_bytes=2 * FB + 1), "records-1frame": dict(stars_rec_bytes=RB),
           "records-2frames": dict(stars_rec_bytes=2 * RB), "records-2-stage-1": dict(stars_rec_bytes=2 * RB, stage_bytes=FB)}[name]
    with open_ctx() as ctx:
        ctx.debug_unit_limits()
        alone = [ctx.find_stars(frames[i:i + 1], sigma=sigma[i:i + 1], max_obj=STARS_OBJ) for i in range(6)]
        assert ctx.debug_unit_split()["chunks"] == 1
        ctx.debug_unit_limits(**lim)
        split = False
        for loc in LOCS:
            for device_out in (False, True):
                what = f"find_stars {loc} records on the {'device' if device_out else 'host'}"
                with located(ctx, loc, frames, be=True) as (f, _, pin):
                    rec, frec = ctx.find_stars(f, sigma=sigma, max_obj=STARS_OBJ, device_out=device_out, **pin)
                    rec = host(rec).view(_native.STAR_DTYPE).reshape(6, STARS_OBJ)
                assert_records((rec, frec), want, what)
                for i in range(6):                                            # what the frame gives alone
                    assert rec[i].tobytes() == alone[i][0][0].tobytes() and frec[i].tobytes() == alone[i][1][0].tobytes(), (what, i)
                # frames per chunk: by the staged bytes of host frames and by the bytes of records that go to the host
                per = 32768
                if loc != "device" and "stage_bytes" in lim:
                    per = min(per, max(1, lim["stage_bytes"] // FB))
                if not device_out and "stars_rec_bytes" in lim:
                    per = min(per, max(1, lim["stars_rec_bytes"] // RB))
                got = ctx.debug_unit_split()
                print(what, lim, got)
                assert got["chunks"] == ceil_div(6, per), (what, lim, got)
                split |= got["chunks"] > 1
        assert split


# ---- stacked cross-sections -------------------------------------------------------------------------------------------------------
STACK_SHAPE = (97, 130)
STACK_ON = (0, 1, 3, 4, 6)    # of seven frames


@functools.lru_cache(maxsize=None)
def stack_case():
    h, w = STACK_SHAPE
    frames = np.stack([TK.dirty(TK.trail_frame(STACK_SHAPE, 20 + k, w / 2, h / 2, 100 if k in (0, 4, 6) else 20), 30 + k) for k in range(7)])
    segs = TK.segment_set(STACK_SHAPE)
    ix = [0, 0]
    for i in range(len(segs)):                                                # frame 0's segments over 0, 4, 6; frame 1's over 1, 3
        which = int(segs["frame"][i])
        segs["frame"][i] = ((0, 4, 6), (1, 3))[which][ix[which] % (3, 2)[which]]
        ix[which] += 1
    sigma = np.linspace(0.025, 0.03, 7).astype(np.float32)
    kw = dict(TK.SMALL, n_iter=1)
    refs = [S.measure(frames[int(s["frame"])], (s["x1"], s["y1"], s["x2"], s["y2"]), sigma[int(s["frame"])], **kw) for s in segs]
    assert sorted({int(s["frame"]) for s in segs}) == list(STACK_ON)
    assert {r[0]["n_pass"] for r in refs} >= {0, 1, 2}                          # some stop after the first pass: the second splits differently
    frozen(frames, segs, sigma)
    return frames, segs, sigma, kw, refs


def stack_blocks(s, shape):
    """blocks of 32 columns a segment takes, its two halves apart (include/lfdmi.h: lfdmi_debug_unit_limits); 0: not measured"""
    h, w = shape
    c = [float(s[k]) for k in ("x1", "y1", "x2", "y2")]
    if not all(math.isfinite(v) for v in c) or (c[0] == c[2] and c[1] == c[3]):
        return 0
    xmajor = abs(c[2] - c[0]) >= abs(c[3] - c[1])
    a1, a2, A = (c[0], c[2], w) if xmajor else (c[1], c[3], h)
    first, last = int(max(math.ceil(min(a1, a2)), 0.0)), int(min(math.floor(max(a1, a2)), A - 1.0))
    return (last >> 5) - (first >> 5) + 2 if last - first + 1 >= TK.SMALL["min_cols"] else 0


def stack_launches(needs, cap):
    """whole segments up to ``cap`` blocks a launch; a launch's first segment always fits"""
    n, inside = 0, 0
    for need in needs:
        if inside == 0 or inside + need > cap:
            n, inside = n + 1, 0
        inside += need
    return n


@pytest.mark.parametrize("loc", LOCS)
def test_stack_profiles_in_groups_of_frames_and_launches(loc):
    frames, segs, sigma, kw, refs = stack_case()
    nb = S.n_bins(kw)
    needs_of = lambda fr: [b for b in (stack_blocks(s, STACK_SHAPE) for s in segs if int(s["frame"]) in fr) if b]  # noqa: E731
    with open_ctx() as ctx:
        for lim in (dict(stage_bytes=2 * frames[0].nbytes), dict(stack_part_bytes=8 * nb * 12),
                    dict(stage_bytes=2 * frames[0].nbytes, stack_part_bytes=8 * nb * 12), dict(stack_part_bytes=1)):
            ctx.debug_unit_limits(**lim)
            with located(ctx, loc, frames, be=True) as (f, _, pin):
                rec, rows, A, N = ctx.stack_profiles(f, segs, sigma=sigma, raw=True, **pin, **kw)
            bad = [msg for msg in (TK.same(i, rec[i], rows[i], A[i], N[i], refs[i]) for i in range(len(segs))) if msg]
            assert not bad, (loc, lim, bad[:5])
            # host frames that carry a segment are staged two at a time: (0, 1), (3, 4), (6); device frames are one group
            staged = loc != "device" and "stage_bytes" in lim
            groups = 3 if staged else 1
            needs = needs_of(STACK_ON[:2] if staged else STACK_ON)
            cap = max(max(needs), max(1, lim["stack_part_bytes"] // (8 * nb))) if "stack_part_bytes" in lim else sum(needs)
            got = ctx.debug_unit_split()
            print(loc, lim, got)
            assert (got["chunks"], got["launches"]) == (groups, stack_launches(needs, cap)), (loc, lim, got)
            if "stack_part_bytes" in lim:
                assert got["launches"] >= 3
            elif loc == "device":
                assert (got["chunks"], got["launches"]) == (1, 1)
            else:
                assert got["chunks"] == 3


# ---- the debug entries themselves -------------------------------------------------------------------------------------------------
def test_the_limits_clamp_restore_stay_in_their_context_and_refuse_in_flight():
    import torch
    from lfd_amd import _native
    from lfd_amd.detecttrails import default_params
    shape = (37, 130)
    segs, _, _, want_mask, _, _ = mask_case(shape)
    unsplit = dict(chunks=1, batches=0, grid=len(CARRY) * tiles(shape), launches=0)

    def split_of(ctx):
        mask, _, _ = ctx.mask_trails(None, segs, shape=(N_FRAMES, *shape))
        TM.assert_equal("mask", mask, want_mask)
        return ctx.debug_unit_split()

    with open_ctx() as ctx, open_ctx() as other:
        zeros = dict(chunks=0, batches=0, grid=0, launches=0)
        ctx.mask_trails(None, segs, shape=(N_FRAMES, *shape))
        assert ctx.debug_unit_split() == zeros              # nothing is kept of a context before it calls one of the two entries
        other.debug_unit_limits()
        assert split_of(ctx) == unsplit
        # a value above the default is clamped to it: today's split
        ctx.debug_unit_limits(list_pairs=1 << 40, stage_bytes=1 << 50, cell_bytes=1 << 50, render_blocks=1 << 30, stars_rec_bytes=1 << 50,
                              stack_part_bytes=1 << 50)
        assert split_of(ctx) == unsplit
        s_segs, s_frames, _, s_want, _, _ = strip_case(shape)                               # ... for the units that read the other kinds
        kw = dict(max_sections=MAX_SEC, max_cells=s_want[2].shape[1])
        TS.assert_all("strips", ctx.trail_strips(s_frames, s_segs, **kw, **TS.PARAMS), s_want)
        assert ctx.debug_unit_split() == dict(unsplit, batches=1)
        u_segs, u_frames, _, u_want, _, _ = sub_case(shape)
        TU.assert_same("sub", ctx.subtract_trails(u_frames.copy(), u_segs, **kw, **TU.PARAMS)[0], u_want[1])
        assert ctx.debug_unit_split() == unsplit
        frames, sigma, want = stars_case()
        assert_records(ctx.find_stars(frames, sigma=sigma, max_obj=STARS_OBJ), want, "stars")
        assert ctx.debug_unit_split() == dict(zeros, chunks=1)
        k_frames, k_segs, k_sigma, k_kw, k_refs = stack_case()
        rec, rows, A, N = ctx.stack_profiles(k_frames, k_segs, sigma=k_sigma, raw=True, **k_kw)
        assert not [m for m in (TK.same(i, rec[i], rows[i], A[i], N[i], k_refs[i]) for i in range(len(k_segs))) if m]
        assert ctx.debug_unit_split() == dict(zeros, chunks=1, launches=1)
        ctx.debug_unit_limits(list_pairs=tiles(shape), render_blocks=2)
        assert split_of(ctx) == dict(unsplit, chunks=len(CARRY), grid=2)
        assert split_of(other) == unsplit                                                   # another context keeps its defaults
        # a negative field is refused and changes nothing; 0 is the default of that field alone
        for k in ("list_pairs", "stage_bytes", "cell_bytes", "render_blocks", "stars_rec_bytes", "stack_part_bytes"):
            with pytest.raises(_native.NativeError) as e:
                ctx.debug_unit_limits(**{k: -1})
            assert e.value.code == _native.ERR_ARG and "lfdmi_debug_unit_limits" in str(e.value)
        assert split_of(ctx) == dict(unsplit, chunks=len(CARRY), grid=2)
        ctx.debug_unit_limits(list_pairs=0, render_blocks=2)
        assert split_of(ctx) == dict(unsplit, grid=2)
        ctx.debug_unit_limits()                                                             # zeros: every default again
        assert split_of(ctx) == unsplit
        ctx.debug_unit_limits(render_blocks=2)
        ctx.debug_unit_limits(forget=True)                                                  # NULL: every default, and nothing kept
        ctx.mask_trails(None, segs, shape=(N_FRAMES, *shape))
        assert ctx.debug_unit_split() == zeros
        assert split_of(ctx) == unsplit
        with pytest.raises(TypeError):
            ctx.debug_unit_limits(no_such_limit=1)
    # both refuse while a call is in flight, like the units
    with _native.Context(0, 97, 130, 2) as ctx:
        pb, pd, _ = default_params()
        dev = torch.zeros((2, 97, 130), dtype=torch.float32, device="cuda")
        pend = ctx.detect_batch_begin(dev, pb, pd)
        for call in (lambda: ctx.debug_unit_limits(render_blocks=1), ctx.debug_unit_limits, ctx.debug_unit_split):
            with pytest.raises(_native.NativeError) as e:
                call()
            assert e.value.code == _native.ERR_ARG
        pend.result()
        ctx.mask_trails(None, segs, shape=(N_FRAMES, *shape))
        assert ctx.debug_unit_split() == zeros                                              # (a refused call opened nothing)
        assert split_of(ctx) == unsplit
