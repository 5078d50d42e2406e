"""The four searches of one Radon handle in turn -- wide, short, lines, plain, lines, short, wide -- against their numpy
restatements, byte for byte: the peeling searches share one round driver and the handle's lazily allocated buffers, so what
this checks is that no mode leaves anything behind for the next (the second V, M set, the rounds' line and width arrays, the
sigma the rounds overwrite), in either order of first calls, from host frames and from a device tensor, through two chunks.

24 x 72 at bin 1: orientations 0 and 1 have P = 128, the smallest width with a scoring level of the short search (min_strip = 64
needs P >= 128); orientations 2 and 3 have P = 32, where the scalar last level runs.  The lines' and the short trails' end
points equal the restatement's to the bit as well, which they only do if a row offset of exactly 0.0 leaves the geometry's
arithmetic what it was."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_lines_ref as L  # noqa: E402
import radon_ref as R  # noqa: E402
import radon_short_ref as S  # noqa: E402
import radon_wide_ref as W  # noqa: E402
import test_gpu_radon as TG  # noqa: E402
import test_gpu_radon_lines as TGL  # noqa: E402
import test_gpu_radon_wide as TGW  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (24, 72)
HANDLE = {"bin": 1, "min_len": 16, "threshold": 6.0}
SIGMA = np.array([0.025, 0.03, 0.02], np.float32)
LINES = {"max_lines": 3, "peel_halfwidth": 2, "min_seg": 16}
SHORT = dict(LINES, min_strip=64, short_threshold=6.0)
WIDE = dict(LINES, max_width=8, wide_threshold=6.0)
ORDER = ("wide", "short", "lines", "plain", "lines", "short", "wide")


def mode_frames():
    """dirty noise alone; a band three cells wide and a streak that crosses it; one streak"""
    f = np.stack([TG.dirty_noise(SHAPE, 61 + k) for k in range(3)])
    TGW.paint_band(f[1], 0, 4, 9, 3, 0.06)
    TGL.streak(f[1], 30, 14, 1.0, -0.2, 0.08)
    TGL.streak(f[2], 40, 10, 1.0, 0.1, 0.07)
    return f


def records(dicts, dtype):
    """the restatement's records (one list of dicts per frame) as the structured array the library fills"""
    out = np.zeros((len(dicts), len(dicts[0])), dtype)
    for i, recs in enumerate(dicts):
        for k, rec in enumerate(recs):
            for name in dtype.names:
                if name in rec:
                    out[i, k][name] = rec[name]
    return out


@functools.lru_cache(maxsize=None)
def restatement():
    """{mode: (records, n_lines[, plain records])} of mode_frames() by the numpy restatements, computed once and only read"""
    from lfd_amd import _native
    frames = mode_frames()
    plain = records([[R.search(f, sg, **HANDLE)] for f, sg in zip(frames, SIGMA)], _native.RADON_DTYPE)[:, 0]
    lines = [L.search_lines(f, sg, **HANDLE, **LINES) for f, sg in zip(frames, SIGMA)]
    short = [S.search_short(f, sg, **HANDLE, **SHORT) for f, sg in zip(frames, SIGMA)]
    wide = [W.search_wide(f, sg, **HANDLE, **WIDE) for f, sg in zip(frames, SIGMA)]

    def peeled(res, dtype):
        out = [records([x[0] for x in res], dtype), np.array([x[1] for x in res], np.int32)]
        if len(res[0]) > 2:
            out.append(records([[x[2]] for x in res], _native.RADON_DTYPE)[:, 0])
        return tuple(out)
    want = {"plain": (plain,), "lines": peeled(lines, _native.RADON_LINE_DTYPE), "short": peeled(short, _native.RADON_SHORT_DTYPE),
            "wide": peeled(wide, _native.RADON_WIDE_DTYPE)}
    for v in want.values():
        for a in v:
            a.setflags(write=False)
    return want


def check_restatement(want):
    """what the frames are there for, on the restatement's own output"""
    for mode in ("lines", "short", "wide"):
        n_lines = want[mode][1]
        assert n_lines.max() >= 2 and n_lines.min() == 0, (mode, n_lines)
    wide, wn = want["wide"][:2]
    assert max(int(wide[i, k]["width"]) for i in range(len(wn)) for k in range(wn[i])) > 1       # the wid path runs
    for mode in ("short", "wide"):
        assert want[mode][2].tobytes() == want["plain"][0].tobytes()


def run(r, mode, frames):
    if mode == "plain":
        return (r.search(frames, sigma=SIGMA),)
    if mode == "lines":
        return r.search_lines(frames, sigma=SIGMA, **LINES)
    if mode == "short":
        return r.search_short(frames, sigma=SIGMA, plain=True, **SHORT)
    return r.search_wide(frames, sigma=SIGMA, plain=True, **WIDE)


def test_the_modes_do_not_interfere_through_the_handle(gpu_ctx):
    import torch
    from lfd_amd import _native
    want = restatement()
    check_restatement(want)
    frames = mode_frames()
    dev_frames = torch.from_numpy(frames).cuda()
    with _native.Radon(gpu_ctx, SHAPE, max_frames=2, **HANDLE) as r, _native.Radon(gpu_ctx, SHAPE, max_frames=2, **HANDLE) as back:
        plain = None
        for turn, mode in enumerate(ORDER):                    # three frames through two slots: two chunks
            got = run(r, mode, dev_frames if turn % 2 else frames)
            assert len(got) == len(want[mode])
            for a, b in zip(got, want[mode]):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (turn, mode)
            if mode == "plain":
                plain = got[0]
        held = r.dims()[2]
        for mode in ("short", "wide"):                          # the plain records of both are search's
            assert run(r, mode, frames)[2].tobytes() == plain.tobytes()
        assert r.dims()[2] == held                              # a repeated call allocates nothing
        # the same calls in the reverse order on a second handle.  ORDER reads the same backwards, so it is taken from its middle:
        # plain, lines, short, wide first -- every buffer's first call comes in the opposite order -- then wide, short, lines
        for turn, mode in enumerate(ORDER[3:] + ORDER[:3]):
            got = run(back, mode, frames if turn % 2 else dev_frames)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want[mode])), (turn, mode)
        assert back.dims()[2] == held
    assert np.array_equal(dev_frames.cpu().numpy().view(np.uint32), frames.view(np.uint32))     # only read
