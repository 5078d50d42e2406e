"""lfdmi_detect_rounds on eight 512 x 768 frames with 0 .. 3 streaks (tests/rounds_cases.py): every field of every record,
n_found and dup_of equal the loop built from existing public calls (tests/rounds_gpu.py), four frames equal tests/rounds_ref.py
on the oracle, record 0 and the caller's frames equal a plain detect_batch, max_trails = 1 is the plain call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounds_cases as RC  # noqa: E402
import rounds_gpu as RG  # noqa: E402
import rounds_ref as RR  # noqa: E402

from lfd_amd import _native, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    frames, cats = RC.frames()
    ctx = _native.Context(0, *RC.SHAPE, 8)
    yield frames, cats, ctx
    ctx.close()


@pytest.mark.parametrize("half", [RC.HALF, 10.0])
def test_equals_the_loop_of_public_calls(world, half):
    frames, cats, ctx = world
    pb, pd, rs, _ = RG.params()
    want = RG.composed(ctx, frames, cats, 4, half)
    work = frames.copy()
    got = ctx.detect_rounds(work, pb, pd, synth.pack_catalogs(cats), rs, max_trails=4, half=half)
    print(got[1].tolist(), got[2].tolist())
    assert RG.same(got, want)
    assert got[1].max() >= 2                                   # (some frame did go into a later round)
    plain_frames = frames.copy()
    plain = ctx.detect_batch(plain_frames, pb, pd, synth.pack_catalogs(cats), rs)
    assert got[0][:, 0].tobytes() == plain.tobytes() and work.tobytes() == plain_frames.tobytes()


def test_four_frames_equal_the_reference_on_the_oracle(world, oracle):
    frames, cats, ctx = world
    pb, pd, rs, prs = RG.params()
    rs_o = oracle.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    idx = [0, 2, 3, 7]
    rec, nf, dup = ctx.detect_rounds(frames[idx].copy(), pb, pd, synth.pack_catalogs([cats[i] for i in idx]), rs, max_trails=4, half=RC.HALF)
    for s, i in enumerate(idx):
        w_rec, w_nf, w_dup = RR.rounds(frames[i], RR.oracle_detect(oracle, pb, pd, cats[i], rs_o), 4, RC.HALF)
        assert int(nf[s]) == w_nf and dup[s].tolist() == w_dup.tolist(), i
        for k in range(4):
            for name in RR.RESULT_DTYPE.names:
                assert rec[s, k][name] == w_rec[k][name], (i, k, name)


def test_one_trail_is_the_plain_call(world):
    frames, cats, ctx = world
    pb, pd, rs, _ = RG.params()
    a, b = frames.copy(), frames.copy()
    rec, nf, dup = ctx.detect_rounds(a, pb, pd, synth.pack_catalogs(cats), rs, max_trails=1)
    plain = ctx.detect_batch(b, pb, pd, synth.pack_catalogs(cats), rs)
    assert rec.shape == (8, 1) and rec[:, 0].tobytes() == plain.tobytes() and a.tobytes() == b.tobytes()
    assert nf.tolist() == [int(RG.found(r)) for r in plain] and dup.tolist() == [[-1]] * 8


def test_the_batch_detector_shards_over_lanes_and_refuses_sky(world):
    from lfd_amd.batch import BatchDetector
    frames, cats, ctx = world
    pb, pd, rs, _ = RG.params()
    want = ctx.detect_rounds(frames.copy(), pb, pd, synth.pack_catalogs(cats), rs, max_trails=3, half=RC.HALF)
    for lanes in (1, 2):
        bd = BatchDetector(0, RC.SHAPE, inflight=8, lanes=lanes)
        try:
            got = bd.detect_rounds(frames.copy(), pb, pd, synth.pack_catalogs(cats), rs, rounds_params={"max_trails": 3, "half": RC.HALF})
        finally:
            bd.close()
        assert RG.same(got, want), lanes
    bd = BatchDetector(0, RC.SHAPE, inflight=8, sky={})
    try:
        with pytest.raises(RuntimeError, match="not routed through sky="):
            bd.detect_rounds(frames.copy(), pb, pd, synth.pack_catalogs(cats), rs)
    finally:
        bd.close()
