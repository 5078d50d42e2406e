"""The hole-border reject test of k_frame_contours (lfd_amd/csrc/hole_prune.h) compiled for the host
(tools/hole_prune_check.cpp, g++) and held against the oracle's own findContours -> minAreaRect -> filter: every hole the
function rejects must be one whose border the oracle's filter rejects, at lwTresh in {0, 1.5, 5} x minAreaRectMinLen in
{0, 1, 3}: every 5 x 5 image, random 24 x 24 and 40 x 64 images, and hand-made holes."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LW, ML = (0.0, 1.5, 5.0), (0.0, 1.0, 3.0)


@pytest.fixture(scope="module")
def checker(oracle, tmp_path_factory):
    so = os.path.join(ROOT, "oracle", "liblfd_oracle.so")
    exe = tmp_path_factory.mktemp("hole_prune") / "hole_prune_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "lfd_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           "-o", str(exe), os.path.join(ROOT, "tools", "hole_prune_check.cpp"), so, "-Wl,-rpath," + os.path.dirname(so)])
    return str(exe)


def summary(out):
    """'images I holes H rejected r0 .. r8 violations V unmatched U' -> dict"""
    t = out.strip().splitlines()[-1].split()
    assert t[0] == "images" and t[2] == "holes" and t[4] == "rejected" and t[14] == "violations" and t[16] == "unmatched", out
    return dict(images=int(t[1]), holes=int(t[3]), rejected=np.array(t[5:14], np.int64).reshape(3, 3), violations=int(t[15]),
                unmatched=int(t[17]))


def run(checker, *args):
    p = subprocess.run([checker, *[str(a) for a in args]], capture_output=True, text=True)
    assert p.returncode in (0, 1), p.stderr
    return p.stdout


@pytest.mark.parametrize("args,images", [(("exhaustive5",), 1 << 25), (("random", 24, 24, 3000, 1), 3000), (("random", 40, 64, 600, 2), 600)],
                         ids=["exhaustive_5x5", "random_24x24", "random_40x64"])
def test_never_rejects_what_the_oracle_accepts(checker, args, images):
    s = summary(run(checker, *args))
    print(s)
    assert s["images"] == images and s["holes"] > 1000
    assert s["unmatched"] == 0, "a hole border of the oracle does not belong to exactly one hole of the image"
    assert s["violations"] == 0
    assert not s["rejected"][0].any(), "lwTresh 0: neither bound holds"
    assert s["rejected"][2, 1] > 0 and (np.diff(s["rejected"][1:], axis=1) >= 0).all() and (s["rejected"][2] >= s["rejected"][1]).all()


def blob(h=24, w=96):
    """All ones: whatever is cut out of it away from the frame is a hole."""
    return np.ones((h, w), np.uint8)


def holes_of(checker, tmp_path, img, name):
    path = tmp_path / (name + ".bin")
    path.write_bytes(struct.pack("<ii", *img.shape) + np.ascontiguousarray(img, np.uint8).tobytes())
    out = run(checker, "file", path)
    s = summary(out)
    assert s["violations"] == 0 and s["unmatched"] == 0, (name, out)
    holes = {}
    for line in out.splitlines():
        t = line.split()
        if t and t[0] == "hole":
            d = dict(zip(t[1::2], t[2::2]))
            holes.setdefault((int(d["x"]), int(d["y"]), int(d["n"]), int(d["wb"]), int(d["hb"])), {})[(float(d["lw"]), float(d["minlen"]))] = \
                (int(d["rejected"]), int(d["oracle_accepts"]))
    return holes


def one_hole(checker, tmp_path, img, name):
    holes = holes_of(checker, tmp_path, img, name)
    assert len(holes) == 1, (name, holes)
    (key, v), = holes.items()
    assert len(v) == 9
    return key, v


def test_hand_made_holes(checker, tmp_path):
    D = (5.0, 1.0)                                           # the default filter
    # a diagonal slit, one pixel wide (a staircase: holes are 4-connected): kept, and the oracle accepts its border
    img = blob(24, 40)
    for i in range(14):
        img[4 + i, 6 + i:8 + i] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "diagonal")
    assert (n, wb, hb) == (28, 16, 15) and v[D] == (0, 1)
    # 1 x 12 slit: kept
    img = blob()
    img[10, 20:32] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "slit")
    assert (x, y, n, wb, hb) == (20, 10, 12, 13, 2) and v[D] == (0, 1)
    # 3 x 3 full hole: rejected (d2 = 32 < 5 * 9)
    img = blob()
    img[10:13, 20:23] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "full3")
    assert (n, wb, hb) == (9, 4, 4) and v[D] == (1, 0) and v[(1.5, 1.0)] == (0, 0) and v[(5.0, 0.0)] == (1, 0)
    # plus-shaped holes: thin ones are kept by the bound although the oracle rejects them (the bound is not tight: 242 against
    # 5 * 36), one with arms four pixels thick is rejected (242 < 5 * 64)
    img = blob()
    img[10, 19:22] = 0
    img[9:12, 20] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "plus1")
    assert (n, wb, hb) == (5, 4, 4) and v[D] == (0, 0)
    img = blob()
    img[10:12, 16:26] = 0
    img[6:16, 20:22] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "plus4")
    assert (n, wb, hb) == (36, 11, 11) and v[D] == (0, 0)
    img = blob()
    img[9:13, 16:26] = 0
    img[6:16, 19:23] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "plus_thick")
    assert (n, wb, hb) == (64, 11, 11) and v[D] == (1, 0)
    # a hole with an island: the island's pixels do not count, the extents are the hole's
    img = blob()
    img[6:15, 20:29] = 0
    img[10, 24] = 1
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "island")
    assert (n, wb, hb) == (80, 10, 10) and v[D] == (1, 0)
    # ... and an elongated one with a long island: kept
    img = blob()
    img[8:13, 10:80] = 0
    img[10, 14:76] = 1
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "island_long")
    assert (n, wb, hb) == (5 * 70 - 62, 71, 6) and v[D] == (0, 1)
    # background touching column 0, row 0 or the last row is not a hole
    for name, sl in (("col0", np.s_[10:13, 0:3]), ("row0", np.s_[0:3, 20:23]), ("lastrow", np.s_[21:24, 20:23])):
        img = blob()
        img[sl] = 0
        assert holes_of(checker, tmp_path, img, name) == {}
    # columns 60 .. 70 (a 64-bit word boundary of the device's bit rows): one row is kept, three rows are rejected
    img = blob()
    img[10, 60:71] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "word1")
    assert (x, n, wb, hb) == (60, 11, 12, 2) and v[D] == (0, 1)
    img = blob()
    img[10:13, 60:71] = 0
    (x, y, n, wb, hb), v = one_hole(checker, tmp_path, img, "word3")
    assert (x, n, wb, hb) == (60, 33, 12, 4) and v[D] == (1, 0)
