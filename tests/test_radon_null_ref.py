"""The hashes of the null peaks (include/lfdmi.h: faint-trail search, null peaks, steps 17, 18) in tests/radon_null_ref.py
against values worked by hand: each constant below was worked with plain integers from the header's text, step by step, and
the first two of each hash are the published vectors of splitmix64 (its first two outputs from state 0) and of murmur3's
finaliser.  The cases are N not a power of two, i = 0, i = N-1 and a key with a zero half; j < N always."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radon_null_ref as N  # noqa: E402

SDSS = 2048 * 1489
# (i, k, N) -> (a, u, j) of step 18
SOURCE_CASES = [
    ((0, 0x6E789E6AA1B965F4, 2800), (0x5542947F, 0xE749C499, 0x9E1)),              # i = 0; 40 x 70
    ((2799, 0x6E789E6AA1B965F4, 2800), (0xDC0E4C77, 0x53B62CE2, 0x393)),           # i = N-1
    ((0, 0x1234567800000000, 8580), (0x0, 0xE37CD1BC, 0x1DC8)),                    # lo32(k) = 0 and i = 0: a = fmix32(0) = 0; 66 x 130
    ((8579, 0x9ABCDEF1, 8580), (0xE8630355, 0x58148675, 0xB88)),                   # hi32(k) = 0, i = N-1
    ((12345, 0x73D33B666A1E21DA, SDSS), (0x8476AA4F, 0x91716C4F, 0x1A6FA5)),       # a whole frame
    ((SDSS - 1, 0x73D33B666A1E21DA, SDSS), (0x1BC2A83C, 0xB093841B, 0x201850)),
    ((5, 0, 7), (0x9982F0BB, 0x7234D648, 3)),                                      # k = 0
]


def test_splitmix64_and_the_key():
    assert N.splitmix64(0) == 0xE220A8397B1DCDAF                   # the generator's first output from state 0
    assert N.splitmix64(N.GOLD64) == 0x6E789E6AA1B965F4            # and its second
    assert N.splitmix64(1) == 0x910A2DEC89025CC1
    assert N.key(0, 0) == 0x6E789E6AA1B965F4                       # seed 0, r = 0: splitmix64(0 + GOLD * 1)
    assert N.key(7, 3) == 0x73D33B666A1E21DA
    assert N.key((1 << 64) - 1, 63) == 0x536703AC09AF3436          # the sum wraps modulo 2^64
    assert len({N.key(s, r) for s in range(8) for r in range(N.NULL_MAX)}) == 8 * N.NULL_MAX


def test_fmix32():
    got = N.fmix32(np.array([0, 1, 0xFFFFFFFF], np.uint32))
    assert got.dtype == np.uint32 and got.tolist() == [0, 0x514E28B7, 0x81F16F39]


@pytest.mark.parametrize("case,want", SOURCE_CASES, ids=["i%d-N%d" % (c[0], c[2]) for c, _ in SOURCE_CASES])
def test_source_pixel(case, want):
    i, k, n = case
    a = N.fmix32(np.array([i], np.uint32) * np.uint32(0x9E3779B1) + np.uint32(k & 0xFFFFFFFF))
    u = N.fmix32(a ^ np.uint32(k >> 32))
    j = N.source(np.array([i], np.uint32), k, n)
    assert (int(a[0]), int(u[0]), int(j[0])) == want
    assert j.dtype == np.uint32 and want[2] == (want[1] * n) >> 32 < n


@pytest.mark.parametrize("n", [1, 7, 2800, 8580, 1 << 16, SDSS])
def test_j_is_always_below_n(n):
    i = np.arange(n, dtype=np.uint32)
    for k in (0, 0x6E789E6AA1B965F4, (1 << 64) - 1, 0xFFFFFFFF00000000):
        j = N.source(i, k, n)
        assert j.dtype == np.uint32 and int(j.max()) < n
    # u = 2^32 - 1 is the largest the product sees
    assert ((0xFFFFFFFF * n) >> 32) < n
    with pytest.raises(ValueError):
        N.source(i[:1], 0, 1 << 32)


def test_scramble_moves_exact_bit_patterns():
    rng = np.random.default_rng(5)
    f = rng.normal(0, 0.025, (40, 70)).astype(np.float32)
    f[0, 0], f[3, 4], f[5, 6], f[7, 8], f[9, 1] = np.nan, np.inf, -0.0, 0.0, 0.5
    f.view(np.uint32)[11, 2] = 0x7FC12345                          # a NaN with a payload
    x = N.scramble(f, 3, 0)
    assert x.shape == f.shape and x.dtype == f.dtype
    j = N.source(np.arange(f.size, dtype=np.uint32), N.key(3, 0), f.size)
    assert np.array_equal(x.view(np.uint32).reshape(-1), f.view(np.uint32).reshape(-1)[j])
    assert set(x.view(np.uint32).reshape(-1).tolist()) <= set(f.view(np.uint32).reshape(-1).tolist())
    # with replacement: not a permutation, and about 1 - 1/e of the pixels are drawn at all
    drawn = np.unique(j).size / f.size
    assert 0.60 < drawn < 0.66
    # another realisation and another seed are other frames; the same pair is the same frame
    assert not np.array_equal(N.scramble(f, 3, 1).view(np.uint32), x.view(np.uint32))
    assert not np.array_equal(N.scramble(f, 4, 0).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(N.scramble(f, 3, 0).view(np.uint32), x.view(np.uint32))
    # a big-endian frame: the stored patterns move, so the values are the same scramble
    be = N.scramble(f.astype(">f4"), 3, 0)
    assert be.dtype == np.dtype(">f4") and np.array_equal(be.astype(np.float32).view(np.uint32), x.view(np.uint32))


def test_scramble_destroys_a_line_and_keeps_the_distribution():
    import radon_ref as R
    f = np.random.default_rng(8).normal(0, 0.025, (64, 96)).astype(np.float32)
    f[30, :] += np.float32(0.05)
    assert R.search(f, bin=1, min_len=32)["found"] == 1
    recs = N.null_records(f[None], 4, bin=1, min_len=32)[0]
    assert all(r["status"] == R.OK and r["found"] == 0 for r in recs)
    assert N.null_snr(f[None], 4, bin=1, min_len=32).shape == (1, 4)


def test_helpers_of_the_package():
    from lfd_amd import radon
    null = np.array([4.5, 5.0, 4.0, 5.5], np.float32)
    assert radon.false_alarm(9.0, null) == 1 / 5 and radon.false_alarm(5.0, null) == 3 / 5 and radon.false_alarm(0.0, null) == 1.0
    assert radon.null_threshold(null) == 1.5 * 5.5 and radon.null_threshold(null, margin=2) == 11.0
    with pytest.raises(ValueError):
        radon.false_alarm(1.0, [])
    assert radon.null_seed(94, 1, "r", 101) == radon.null_seed(94, 1, 2, 101) != radon.null_seed(94, 1, "r", 102)
    assert 0 <= radon.null_seed(94, 1, "r", 101) < 1 << 64
    row = radon.format_null_row((94, 1, "r", 101), "lines", null)
    assert row == "94 1 r 101 lines 4 4.0 4.75 5.5"
    row = radon.format_fap_row((94, 1, "r", 101), "wide", 1, np.float32(5.25), null)
    assert row == "94 1 r 101 wide 1 5.25 1 4 0.4"
