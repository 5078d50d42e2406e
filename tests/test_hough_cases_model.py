"""CPU checks of tests/hough_cases.py: every named case reaches the launch shape it is named for, the cases together cover the
slab widths, slab counts, chunk classes and list splits of k_hough_vote, and the float32 restatement of the kernel's per-chunk
decision gives the oracle's accumulator -- while five deliberately wrong restatements do not."""
import numpy as np
import pytest

import hough_cases as H

MODEL_CASES = ["aw32_r1_runs", "aw16_r1_rand", "aw8_r1_w64k", "aw8_r1_w64k1", "aw8_r1_w64k63", "aw32_r5_runs", "r2", "r4", "r8", "r16", "r32_thin", "r64_thin",
               "r100_thin", "r100_thin_full", "r3", "r20_class_b", "r64_thin_full", "r64_tall", "t_aw32_r4_walk", "t_aw64_r8_walk", "th90", "th360", "th1024_r4"]
# wrong restatement -> the case meant to notice it
WRONG = {"t_off_by_one": "aw32_r5_runs", "wrong_side": "r8", "half_up": "r4", "cross_word": "aw32_r5_runs", "b_on_class_a": "r20_class_b"}


@pytest.fixture(scope="module")
def ref(oracle):
    """oracle accumulators of the model cases, computed once, before any wrong restatement runs"""
    out = {}
    for name in MODEL_CASES:
        c = H.BY_NAME[name]
        out[name] = oracle.hough_accum(H.frame(c), c["rho"], c["theta"])
        out[name].setflags(write=False)
    return out


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c["name"])
def test_case_lands_on_its_launch_shape(case):
    s = H.vote_shape(case["h"], case["w"], case["rho"], case["theta"])
    e = case["expect"]
    got = dict(awl=s["aw_log2"], slabs=s["nslabs"], nbmax=s["nbmax"], cm_a=s["cm_a"], cm_b=s["cm_b"], cls_b=s["cls_b"])
    assert got == e
    assert s["fits"] and s["per_slab"] == (s["nslabs"] <= H.VOTE_MAX_SLABS) and s["numangle"] <= H.MAX_ANGLES
    assert s["nsplit"] == 4 and s["balance"] == 0                       # one frame, one image: the default four pieces
    assert max(case["h"], case["w"]) <= 8191 and case["h"] * case["w"] <= 150_000
    assert (s["numangle"] + 2) * (s["numrho"] + 2) * 4 <= 25e6
    if s["per_slab"]:                                                   # every slab's rows inside the accumulator, its LDS slab inside nbmax
        half = (s["numrho"] - 1) // 2                                   # (bins -1 and numrho, the guard cells, included)
        assert all(-half - 1 <= lo <= hi <= s["numrho"] - half and hi - lo + 1 <= s["nbmax"] for lo, hi in zip(s["lo"], s["hi"]))
    else:
        assert s["nbmax"] == s["numrho"] + 2 and s["cm_b"] == 0 and s["cls_b"] == 0
    assert (s["cm_b"] > 0) == (s["cls_b"] != 0) and (s["cm_b"] == 0 or s["cm_b"] >= 2 * s["cm_a"])
    h, w = H.ctx_dims(case)
    assert (s["numangle"] + 2) * (s["numrho"] + 2) <= 182 * (2 * (h + w) + 3)


def test_cases_cover_the_launch_shapes():
    shapes = {c["name"]: H.vote_shape(c["h"], c["w"], c["rho"], c["theta"]) for c in H.CASES}
    assert {s["aw_log2"] for s in shapes.values()} == {1, 2, 3, 4, 5, 6}          # (AWL 0: numrho > 19 400, two sides near 8191)
    for awl in range(1, 7):                                                      # each width with ranges where they exist ...
        if awl > 1:
            assert any(s["aw_log2"] == awl and s["per_slab"] for s in shapes.values()), awl
    assert {s["aw_log2"] for s in shapes.values() if not s["per_slab"]} >= {1, 2, 5, 6}   # ... and without
    assert {32, 64} <= {s["nslabs"] for s in shapes.values()}                     # the last count with ranges, and beyond
    for awl in (3, 4, 5):                                                        # chunks longer than a pixel under SUBS > 1
        assert any(s["aw_log2"] == awl and s["cm_a"] > 1 and s["cm_b"] > 0 for s in shapes.values()), awl
    assert {s["cm_a"] for s in shapes.values()} >= {1, 2, 3, 4, 5, 8, 16, 20, 32, 64}
    assert any(s["cm_b"] == 0 for s in shapes.values()) and {s["cm_b"] for s in shapes.values()} >= {2, 4, 6, 7, 10, 12, 46}
    assert any(c["rho"] == 20 and shapes[c["name"]]["cls_b"] for c in H.CASES) and any(c["rho"] == 5 and shapes[c["name"]]["cls_b"] for c in H.CASES)
    assert {8191} <= {c["w"] for c in H.CASES} and {8191} <= {c["h"] for c in H.CASES}
    assert {0, 1, 63} <= {c["w"] % 64 for c in H.CASES if c["frame"] == "edge"}
    assert {c["frame"] for c in H.CASES} >= {"full", "rows", "runs", "edge", "corners", "empty", "rand"}
    assert {c["div"] for c in H.CASES} >= {90, 180, 360, 1024, 2048, 4096}
    assert sum(c["h"] > c["w"] for c in H.CASES) >= 3


def test_variants_cover_the_splits_and_the_balance():
    c = H.BY_NAME["aw16_r5_runs"]
    got = {vid: H.variant_shape(c, env) for vid, env in H.VARIANTS}
    assert {s["nsplit"] for s in got.values()} == {1, 2, 4, 8, 16}
    assert got["classes0"]["cm_b"] == 0 and got["classes0"]["cls_b"] == 0 and got["default"]["cls_b"] != 0
    assert all(s["aw_log2"] == got["default"]["aw_log2"] and s["cm_a"] == got["default"]["cm_a"] for s in got.values())
    # two images: a pool of 2 * nsplit pieces per slab shared out by list length, unless the lists are not split or the switch is off
    for split, bal_env, want in ((1, "1", (1, 0, 1)), (2, "1", (2, 1, 4)), (4, "1", (4, 1, 8)), (16, "1", (16, 1, 32)), (4, "0", (4, 0, 4)), (3, "1", (4, 1, 8))):
        s = H.vote_shape(300, 400, 5, vote_split=split, n_img=2, balance=bal_env != "0")
        assert (s["nsplit"], s["balance"], s["vsplit"]) == want
    assert H.vote_shape(1489, 2048, 20, n_img=2, nc=256)["nsplit"] == 4 and H.vote_shape(1489, 2048, 20, n_img=2, nc=512)["nsplit"] == 2


def test_run_frames_hold_every_length_at_every_bit_offset():
    c = H.BY_NAME["aw16_r5_runs"]
    placed = H.runs_placed(c["h"] - 2, c["w"])
    assert {(ln, x % 64) for _, x, ln in placed} == {(ln, off) for ln in H.RUN_LENGTHS for off in H.RUN_OFFSETS}
    img = H.frame(c)
    y, x0, ln = H.chunk_list(img, 64)
    assert ln.max() == 64 and ((x0 % 64) + ln <= 64).all()                      # full words; no chunk leaves its word
    assert ((x0 % 64 == 0) & (ln == 64)).any() and ((x0 + ln) % 64 == 0).any()
    for cm in (1, 5, 12, 64):                                                   # every list holds every pixel once
        y, x0, ln = H.chunk_list(img, cm)
        assert ln.sum() == np.count_nonzero(img) and ln.min() >= 1 and ln.max() <= cm
    for name in ("aw8_r1_w64k", "aw8_r1_w64k1", "aw8_r1_w64k63", "w8191_r1"):    # runs that end in the last column
        c = H.BY_NAME[name]
        y, x0, ln = H.chunk_list(H.frame(c), 64)
        assert (x0 + ln == c["w"]).sum() == c["h"] and (x0 == 0).sum() == c["h"]


def test_every_outcome_of_the_vote_decision_occurs():
    """one bin / estimate exact / one-pixel correction in both directions / exact walk, with one chunk per step (AW 64) and
    with several (AW < 64).  The walk needs a chunk across an odd half bin at the table's 90-degree entry: the tall cases."""
    seen = {1: dict.fromkeys(H.OUTCOMES, 0), 2: dict.fromkeys(H.OUTCOMES, 0)}
    for c in H.CASES:
        if c["rho"] == 1 or c["h"] * c["w"] > 70_000:
            continue
        s = H.vote_shape(c["h"], c["w"], c["rho"], c["theta"])
        for k, v in H.outcome_counts(H.frame(c), s, limit=1 << 17).items():
            seen[1 if s["subs"] == 1 else 2][k] += v
    for subs in (1, 2):
        assert all(seen[subs][k] > 0 for k in H.OUTCOMES), (subs, seen[subs])


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_accumulator_equals_the_oracle(ref, name):
    c = H.BY_NAME[name]
    s = H.vote_shape(c["h"], c["w"], c["rho"], c["theta"])
    assert np.array_equal(H.accumulate(H.frame(c), s), ref[name])
    if s["cm_b"]:                                                              # ... whichever list a slab votes with
        assert np.array_equal(H.accumulate(H.frame(c), H.variant_shape(c, {"LFDMI_VOTE_CLASSES": "0"})), ref[name])


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_a_wrong_restatement_changes_the_accumulator(ref, wrong):
    c = H.BY_NAME[WRONG[wrong]]
    s = H.vote_shape(c["h"], c["w"], c["rho"], c["theta"])
    got = H.accumulate(H.frame(c), s, wrong=wrong)
    assert got.shape == ref[c["name"]].shape and not np.array_equal(got, ref[c["name"]])


def test_thin_cases_vote_into_the_guard_bins(oracle):
    """numrho = round((2 (w + h) + 1) / rho) holds every bin only while both sides are longer than rho.  On a 16 x 4000 frame at
    rho = 100 (numrho 80, bins -39 .. 40) the pixels beyond x = 3950 round to bin -40 at 172 .. 179 degrees: OpenCV's loop, and
    the oracle with it, counts them in the guard cell in front of the row, where bin -39's neighbour comparison reads them.
    The slab ranges therefore reach from bin -1 to bin numrho; the *_thin cases are the ones that put votes there (and the
    model, which indexes like OpenCV, agrees with the oracle on them: test_model_accumulator_equals_the_oracle)."""
    guard = {}
    for c in H.CASES:
        acc = oracle.hough_accum(H.frame(c), c["rho"], c["theta"])
        assert not acc[0].any() and not acc[-1].any(), c["name"]                  # (the angle guards stay empty)
        guard[c["name"]] = (int(acc[:, 0].sum()), int(acc[:, -1].sum()))
        s = H.vote_shape(c["h"], c["w"], c["rho"], c["theta"])
        half = (s["numrho"] - 1) // 2
        if s["per_slab"]:                                                         # every slab that has guard votes has the guard row
            AW = 1 << s["aw_log2"]
            for sl in range(s["nslabs"]):
                if acc[1 + sl * AW:1 + (sl + 1) * AW, 0].any():
                    assert s["lo"][sl] == -half - 1, (c["name"], sl)
                if acc[1 + sl * AW:1 + (sl + 1) * AW, -1].any():
                    assert s["hi"][sl] == s["numrho"] - half, (c["name"], sl)
    assert guard["r100_thin"][0] == 1021 and guard["r100_thin_full"][0] > 1000
    assert {n for n, g in guard.items() if any(g)} >= {"r100_thin", "r100_thin_full", "r64_thin_full"}
    assert not any(guard["r64_tall"]) and not any(guard["aw8_r1_full"])


def test_no_vote_leaves_the_guard_bins():
    """The slab rows end at bins -1 and numrho; a vote beyond them would be an LDS add outside the slab.  A pixel's bin is
    monotone in x and in y at every angle (float32 products and sums are), so the four corner pixels bound every vote: for each
    case, and for thin shapes at rhos up to far more than the short side, no corner's bin leaves -1 .. numrho
    (|r| - (numrho - 1) / 2 < 1.75 - (h + 1.5) / rho)."""
    shapes = [(c["h"], c["w"], c["rho"], c["theta"]) for c in H.CASES]
    shapes += [(h, w, rho, H.DEG) for h in (1, 2, 3, 16, 40) for w in (1, 7, 100, 999, 1000, 4000, 8191)
               for rho in (1, 1.5, 2, 7.5, 20, 32, 64, 100, 333, 1000, 5000)]
    shapes += [(w, h, rho, H.DEG) for h in (1, 16) for w in (100, 4000, 8191) for rho in (20, 64, 100, 1000)]
    for h, w, rho, theta in shapes:
        na, nr = H.hough_dims(h, w, rho, theta)
        if nr < 1:
            continue                                                            # (refused by the library: no accumulator)
        cos, sin = H.trig_table(na, rho, theta)
        y, x = np.array([0, 0, h - 1, h - 1]), np.array([0, w - 1, 0, w - 1])
        b0 = H.vote_model(y, x, np.ones(4, np.int64), cos, sin)[0]
        half = (nr - 1) // 2
        assert -half - 1 <= b0.min() and b0.max() <= nr - half, (h, w, rho, int(b0.min()), int(b0.max()), half, nr)
