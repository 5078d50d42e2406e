"""lfdmi_stack_profiles with more bins than a workgroup has lanes: prof_half 36 at step 0.25 gives 289 bins, so the bin loops
of k_stack_block and k_stack_combine (k += STK_THREADS, 256) take a second trip, and the window of a bin lies more than 128 bin
widths from the line.  Records, rows, raw sums and counts against the restatement (tests/stack_ref.py) bit for bit, as in
tests/test_gpu_stack.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stack_ref as S  # noqa: E402
import test_gpu_stack as TS  # noqa: E402

pytestmark = pytest.mark.gpu

STK_THREADS = 256
WIDE = dict(TS.SMALL, prof_half=36.0, step=0.25)


@pytest.mark.parametrize("shape", [(97, 130), (130, 97)], ids=["97x130", "130x97"])
def test_289_bins_equal_the_restatement(gpu_ctx, shape):
    """the band is wider than these frames on both sides of most segments: bins without a pixel are part of the comparison"""
    assert S.n_bins(WIDE) == 289 > STK_THREADS and WIDE["prof_half"] + WIDE["step"] / 2 <= 40.0
    frames = TS.two_frames(shape)
    keep = frames.copy()
    segs = TS.segment_set(shape)[:14]
    sigma = np.array([0.025, 0.03], np.float32)
    for n_iter in (0, 2):
        kw = dict(WIDE, n_iter=n_iter)
        rec, rows, A, N = gpu_ctx.stack_profiles(frames, segs, sigma=sigma, raw=True, **kw)
        assert rec.shape == (14,) and rows.shape == (14, 289) and A.shape == N.shape == (14, 2, 289)
        bad, second_trip, far = [], 0, 0
        for i, s in enumerate(segs):
            ref = S.measure(frames[int(s["frame"])], (s["x1"], s["y1"], s["x2"], s["y2"]), sigma[int(s["frame"])], **kw)
            msg = TS.same(i, rec[i], rows[i], A[i], N[i], ref)
            if msg:
                bad.append(msg)
            assert ref[0]["status"] in (S.OK, S.TOO_FAINT)
            second_trip += int((ref[3][:, STK_THREADS:] > 0).any())
            far += int((ref[3][:, :144 - 128] > 0).any())
        assert not bad, bad[:5]
        # by the restatement: bins of the second trip hold pixels, and so do bins more than 128 below the centre bin
        assert second_trip > 0 and far > 0, (second_trip, far)
    assert np.array_equal(frames.view(np.uint32), keep.view(np.uint32))                      # only read
