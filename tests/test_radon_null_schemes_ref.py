"""The null schemes and the peel rounds (include/lfdmi.h: faint-trail search, null peaks, steps 21 - 22) in
tests/radon_null_schemes_ref.py: known answers on tiny frames, without a GPU -- the sign flip changes sign bits only and keeps
every count, every shifted row and column is a rotation of the original, the offsets stay below the size at W = 1 and H = 1, the
scramble through this restatement is radon_null_ref's, and a peeled round has no more pixels on a line through the band."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_lines_ref as L  # noqa: E402
import radon_null_ref as NR  # noqa: E402
import radon_null_schemes_ref as NS  # noqa: E402
import radon_ref as R  # noqa: E402
from test_gpu_radon_null import planted  # noqa: E402


@pytest.mark.parametrize("order", ["<f4", ">f4"])
def test_signflip_changes_sign_bits_only_and_keeps_every_count(order):
    """the planted frames: NaN payloads, +-inf, +-0, |x| = clip"""
    flipped = 0
    for seed, value in ((1, None), (2, 1.0 / 64), (3, -1.0 / 64), (4, None)):
        f = planted((66, 130), seed, value)
        x = f.astype(order)
        for r in range(3):
            y = NS.null_frame(x, seed, r, "signflip")
            assert y.dtype == x.dtype and y.shape == x.shape
            a, b = f.view(np.uint32), y.astype("<f4").view(np.uint32)
            assert not ((a ^ b) & np.uint32(0x7FFFFFFF)).any()                       # every other bit is kept
            k = NR.key(seed, r)
            assert np.array_equal((a ^ b) >> np.uint32(31), (NS.u_of(np.arange(f.size, dtype=np.uint32), k) >> np.uint32(31)).reshape(f.shape))
            flipped += int(((a ^ b) >> np.uint32(31)).sum())
            for b_ in (1, 2, 4):
                assert np.array_equal(R.prepare(y.astype(np.float32), b_, 0.125)[1], R.prepare(f, b_, 0.125)[1])
            assert np.array_equal(NS.null_frame(f, seed, r, "signflip").view(np.uint32), b)      # either byte order: the same values
    assert 0.45 < flipped / (12 * 66 * 130) < 0.55


def test_u_is_step_18s():
    """u(i) of the schemes is the u from which step 18 takes its source pixel"""
    k = NR.key(5, 2)
    i = np.arange(1000, dtype=np.uint32)
    n = 1000
    assert np.array_equal(((NS.u_of(i, k).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.uint32), NR.source(i, k, n))


def test_every_shifted_row_and_column_is_a_rotation():
    x = np.arange(35, dtype=np.float32).reshape(5, 7) + 1
    for r in range(8):
        k = NR.key(3, r)
        y = NS.null_frame(x, 3, r, "rowshift")
        o = NS.offsets(5, k, 7)
        assert all(np.array_equal(y[i], np.roll(x[i], -int(o[i]))) for i in range(5)) and (o < 7).all()
        assert all(y[i, 0] == x[i, o[i]] for i in range(5))                          # X'[r][c] = X[r][(c + o(r)) mod W]
        y = NS.null_frame(x, 3, r, "colshift")
        o = NS.offsets(7, k, 5)
        assert all(np.array_equal(y[:, c], np.roll(x[:, c], -int(o[c]))) for c in range(7)) and (o < 5).all()
        assert all(y[0, c] == x[o[c], c] for c in range(7))
    offs = {tuple(NS.offsets(5, NR.key(3, r), 7)) for r in range(8)}
    assert len(offs) == 8 and any(len(set(o)) > 1 for o in offs)                     # rows move apart, realisations differ
    be = x.astype(">f4")
    assert np.array_equal(NS.null_frame(be, 3, 0, "rowshift").astype(np.float32), NS.null_frame(x, 3, 0, "rowshift"))


def test_offsets_stay_below_a_size_of_one():
    for r in range(4):
        k = NR.key(1, r)
        assert not NS.offsets(9, k, 1).any()
        col = np.arange(9, dtype=np.float32).reshape(9, 1)
        assert np.array_equal(NS.null_frame(col, 1, r, "rowshift"), col)             # W = 1: o < W is 0
        assert np.array_equal(NS.null_frame(col.T.copy(), 1, r, "colshift"), col.T)  # H = 1
    assert int(NS.offsets(1 << 12, NR.key(2, 0), 1489).max()) < 1489


def test_scramble_through_this_restatement_is_radon_null_refs():
    rng = np.random.default_rng(0)
    f = rng.normal(0, 0.025, (2, 40, 70)).astype(np.float32)
    for kind, kw in (("lines", {}), ("short", {"short_threshold": 3.0, "min_seg": 8}), ("wide", {"wide_threshold": 3.0, "min_seg": 8, "max_width": 4})):
        got = NS.null_records(f, 2, kind, [0.025, 0.03], seeds=[4, 9], bin=1, min_len=20, **kw)
        want = NR.null_records(f, 2, kind, [0.025, 0.03], seeds=[4, 9], bin=1, min_len=20, **kw)
        for a, b in zip(sum(got, []), sum(want, [])):
            assert a.keys() == b.keys()
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), kind


def test_a_peeled_round_has_no_more_pixels_on_a_line_through_the_band():
    rng = np.random.default_rng(7)
    f = rng.normal(0, 0.025, (48, 80)).astype(np.float32)
    for x in range(80):
        f[10 + x // 4, x] += 0.1
    hp = {"bin": 1, "min_len": 16, "threshold": 6.0}
    recs, nl = L.search_lines(f, 0.025, max_lines=2, peel_halfwidth=2, min_seg=8, **hp)
    assert nl >= 1
    line = recs[0]
    peel = NS.peel_of([recs], [nl], 1)[0]
    assert peel == [{"q": line["q"], "y0": line["y0"], "s": line["s"], "width": 1}]
    x = NS.null_frame(f, 0, 0, "signflip")
    V, M = R.prepare(x, 1, 0.125)
    Vp, Mp = NS.peeled(V, M, peel, 2)
    for q in range(4):
        N, Np = R.transform(R.orient(M, q)), R.transform(R.orient(Mp, q))
        assert (Np <= N).all()
    q = line["q"]
    N, Np = R.transform(R.orient(M, q)), R.transform(R.orient(Mp, q))
    P = N.shape[1]
    assert Np[line["y0"] + P - 1, line["s"]] == 0 < N[line["y0"] + P - 1, line["s"]]      # the line itself is gone
    assert int(Mp.sum()) < int(M.sum()) and not Vp[Mp == 0].any()
    # round 1's null record is the search of exactly these arrays, and round 0's of the unpeeled ones
    r1 = NS.null_record(f, 0, 0, "lines", 0.025, "signflip", peel, peel_halfwidth=2, **hp)
    assert r1 == {k: v for k, v in L.search_vm(Vp, Mp, np.float32(0.025), f.shape, dict(R.DEFAULTS, **hp)).items() if k in NR.PLAIN_FIELDS}
    r0 = NS.null_record(f, 0, 0, "lines", 0.025, "signflip", **hp)
    assert r0 == R.search(x, 0.025, **hp)
    # a record of width 0 is no line; peel records need the sign flip and stay in range
    assert NS.null_record(f, 0, 0, "lines", 0.025, "signflip", [{"q": 0, "y0": 0, "s": 0, "width": 0}], **hp) == r0
    for scheme in ("scramble", "rowshift", "colshift"):
        with pytest.raises(ValueError):
            NS.null_record(f, 0, 0, "lines", 0.025, scheme, peel, **hp)
    for bad in ({"q": 4}, {"width": 3}, {"width": 32}, {"s": 128}, {"y0": 48}, {"y0": -128}):
        with pytest.raises(ValueError):
            NS.null_record(f, 0, 0, "lines", 0.025, "signflip", [dict(peel[0], **bad)], **hp)
    with pytest.raises(ValueError):
        NS.null_record(f, 0, 0, "lines", 0.025, "signflip", peel * 9, **hp)


def test_rounds_are_nan_where_the_frame_never_ran_them():
    rng = np.random.default_rng(8)
    f = rng.normal(0, 0.025, (2, 40, 70)).astype(np.float32)
    for x in range(70):
        f[1, 5 + x // 3, x] += 0.1
    hp = {"bin": 1, "min_len": 16, "threshold": 6.0}
    out = [L.search_lines(g, 0.025, max_lines=3, peel_halfwidth=2, min_seg=8, **hp) for g in f]
    lines, nl = [o[0] for o in out], [o[1] for o in out]
    assert nl[0] == 0 and nl[1] >= 1
    rounds = NS.null_rounds(f, lines, nl, 2, "lines", 0.025, peel_halfwidth=2, **hp)
    assert rounds.shape == (2, 3, 2)
    assert np.array_equal(np.isnan(rounds[:, :, 0]), np.arange(3)[None, :] > np.array(nl)[:, None])
    assert np.array_equal(rounds[:, 0], NS.null_snr(f, 2, "lines", 0.025, scheme="signflip", **hp))
    assert np.array_equal(rounds[1, 1], NS.null_snr(f[1:], 2, "lines", 0.025, seeds=[1], scheme="signflip", peel=NS.peel_of(lines[1:], nl[1:], 1),
                                                    peel_halfwidth=2, **hp)[0])
