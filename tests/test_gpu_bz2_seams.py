"""The device bzip2 decoder (lfdmi_bz2_decode_batch: k_bz2.h, bz2_core.h, bz2dev.hip) on the crafted files of tests/bz2_cases.py:
what libbz2's own compressor never writes (code lengths up to 20, incomplete tables, full blocks, spare selectors) and what it
writes on a kernel seam only by chance (a magic at every bit residue, runs against the 256-byte staging buffer, orig_ptr on a
splitter, a head stretch of exactly BZ_SEG_CAP steps, a count byte on a stretch or tile start, a tile's output against BZ_OUTW).
The oracle is libbz2 (Python's ``bz2``); tests/test_bz2_cases_model.py proves on the CPU that every case sits on its seam.  A
"decode" case must come back with status 0 and libbz2's bytes; a "decline_or_equal" one with a non-zero status or libbz2's bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bz2_cases as B  # noqa: E402

pytestmark = pytest.mark.gpu
HEAD = 64


@pytest.fixture(scope="module")
def cases():
    return B.cases()


@pytest.fixture(scope="module")
def decoder():
    from lfd_amd import _native as Nv
    with Nv.Bz2Decoder(0) as z:
        yield z


def pack(blobs):
    off, cur = [], 0
    for c in blobs:
        off.append(cur)
        cur += (len(c) + 7) & ~7
    src = np.zeros(max(cur, 8), np.uint8)
    for o, c in zip(off, blobs):
        src[o:o + len(c)] = np.frombuffer(c, np.uint8)
    return src, off, [len(c) for c in blobs]


def failures(z, cs):
    """Decodes the cases as one batch; one line per case that is not what it has to be."""
    from lfd_amd import _native as Nv
    out_cap = max(len(c.intended) for c in cs) + 4096
    out_len, status, heads = z.decode(*pack([c.data for c in cs]), out_cap, HEAD)
    bad = []
    for i, c in enumerate(cs):
        st = int(status[i])
        what = f"{c.name} [{c.family}: {c.seam}] status {st} ({Nv.BZ2_STATUS.get(st)})"
        if st != 0:
            if c.expect == "decode":
                bad.append(what + ": declined")
            continue
        if c.want is None:
            bad.append(what + f": decoded {int(out_len[i])} bytes of a file that libbz2 rejects")
            continue
        if int(out_len[i]) != len(c.want):
            bad.append(what + f": {int(out_len[i])} bytes, libbz2 {len(c.want)}")
            continue
        got = z.fetch(i, 0, len(c.want)) if c.want else np.zeros(0, np.uint8)
        diff = np.flatnonzero(got != np.frombuffer(c.want, np.uint8))
        if len(diff):
            bad.append(what + f": first differing offset {int(diff[0])} of {len(c.want)}")
        elif heads[i].tobytes() != c.want[:HEAD].ljust(HEAD, b"\0"):
            bad.append(what + ": heads differ")
    return bad


def test_every_case_in_one_batch_then_in_reverse_on_the_same_handle(decoder, cases):
    bad = failures(decoder, cases)
    assert not bad, "\n".join(bad)
    bad = failures(decoder, cases[::-1])
    assert not bad, "\n".join(bad)


def test_every_case_in_several_passes(decoder, cases, monkeypatch):
    """$LFDMI_BZ2_MAX_BLOCKS below the batch's ~630 blocks: groups of whole files, the tables reused from pass to pass."""
    monkeypatch.setenv("LFDMI_BZ2_MAX_BLOCKS", "48")
    bad = failures(decoder, cases)
    assert not bad, "\n".join(bad)


def test_a_block_that_ends_after_four_equal_bytes_is_declined(decoder, cases):
    """libbz2 rejects it ("Invalid data stream"); the run-length kernels used to drop the open count and report status 0."""
    from lfd_amd import _native as Nv
    c = next(c for c in cases if c.name == "ends_in_four")
    assert c.want is None
    _, status, _ = decoder.decode(*pack([c.data]), 4096)
    assert int(status[0]) == 4, Nv.BZ2_STATUS.get(int(status[0]))
