"""The chunk pipeline of detecttrails.py on the CPU: process_field, process_loaded and process_fields_batched over the same eight
frames against a fake context whose records are read off the pixels.  What each frame becomes (sky row, results row or errors
entry, profiles row with its defocus tee or the measurement's errors entry), the order of the rows and the two fallback ladders
(a failed group call: frame by frame from pinned memory, the call's exception for every frame of a device chunk) are host logic.

Pixels the fakes read: [0, 0] > 0 = found, [0, 1] = status, [0, 2] != 0 fails a call of more than one frame, [0, 3] != 0 fails
measure_trails, [0, 4] = the sky value; [1, 0], [1, 1] = rho, theta; row 2 = the profile."""
import contextlib
import os
import re

import numpy as np
import pytest

from lfd_amd import _native
from lfd_amd.catalogs import pack_catalogs
from lfd_amd.detecttrails import default_params, detecttrails, fitslite, loader, sdssfiles

SHAPE = (8, 9)
HDR = {"TAI": 4.5e9, "CRPIX1": 1025.0, "CRPIX2": 745.0, "CRVAL1": 10.5, "CRVAL2": -1.25,
       "CD1_1": 1e-4, "CD1_2": 2e-5, "CD2_1": -2e-5, "CD2_2": 1e-4}
# the caller's order is not the slot order: the loader gives frames of one filter neighbouring slots
#       key                 what                          slot
FRAMES = [((94, 1, "r", 100), "detected", 0),
          ((94, 1, "g", 100), "detected", 5),             # second filter, the slot next to the last r frame
          ((94, 1, "r", 101), "undetected", 1),
          ((94, 1, "r", 102), "nolines", 2),
          ((94, 1, "r", 103), "capacity", 3),
          ((94, 1, "r", 104), "missing", None),           # no file: error[i]
          ((94, 1, "r", 105), "array", None),             # another shape: array[i], the per-frame path
          ((94, 1, "r", 106), "detected", 4)]
KEYS = [f[0] for f in FRAMES]
DETECTED = [k for k, what, _ in FRAMES if what in ("detected", "array")]
GROUP_FAIL, MEASURE_FAIL = 2, 3                           # columns of row 0


def _frame(j, what, flags):
    img = np.zeros((7, 9) if what == "array" else SHAPE, np.float32)
    img[0, 0] = 1.0 if what in ("detected", "array") else 0.0
    img[0, 1] = {"nolines": _native.ERR_NOLINES, "capacity": _native.ERR_CAPACITY}.get(what, 0)
    for col in flags:
        img[0, col] = 1.0
    img[0, 4] = 100.0 + j
    img[1, 0], img[1, 1] = 3.0 + j, 0.25 + 0.125 * j
    img[2, :5] = np.arange(5) + 0.5 * j
    return img


@pytest.fixture
def tree(tmp_path, monkeypatch):
    """write(flags) -> a small SDSS tree of FRAMES; flags: {key: columns of row 0 to set}"""
    redux = tmp_path / "photo" / "redux"
    redux.mkdir(parents=True)
    (redux / "runList.par").write_text(
        "typedef struct {\n int run;\n char rerun[];\n int exist;\n int done;\n int calib;\n"
        " int startfield;\n int endfield;\n char machine[];\n char disk[];\n} RUNDATA;\n\nRUNDATA 94 301 1 1 1 100 107 m d\n")
    monkeypatch.setenv("PHOTO_REDUX", str(redux))
    monkeypatch.setenv("BOSS_PHOTOOBJ", str(tmp_path / "photoObj"))
    sdssfiles._runlist_cache.clear()

    def write(flags=None):
        for j, (key, what, _) in enumerate(FRAMES):
            run, camcol, flt, field = key
            ppath = sdssfiles.filename("photoObj", run, camcol, field)
            os.makedirs(os.path.dirname(ppath), exist_ok=True)
            fitslite.write_table(ppath, {"OBJC_TYPE": np.zeros(1, np.int32), "TYPE": np.zeros((1, 5), np.int32),
                                         "ROWC": np.ones((1, 5), np.float32), "COLC": np.ones((1, 5), np.float32),
                                         "PETROTH90": np.ones((1, 5), np.float32), "PSFMAG": np.ones((1, 5), np.float32),
                                         "NOBSERVE": np.ones(1, np.int32), "NDETECT": np.ones(1, np.int32)})
            if what != "missing":
                fpath = sdssfiles.filename("frame", run, camcol, field, flt)
                os.makedirs(os.path.dirname(fpath), exist_ok=True)
                fitslite.write_image(fpath, _frame(j, what, (flags or {}).get(key, ())), HDR)
    yield write
    sdssfiles._runlist_cache.clear()


class StubDeviceFrames:
    """stands in for _native.DeviceFrames: the big-endian slots, "on the device\""""

    def __init__(self, host):
        self.host, self.shape = host, host.shape

    def slice(self, a, b):
        return StubDeviceFrames(self.host[a:b])


def _host(frames):
    f = frames.host if isinstance(frames, StubDeviceFrames) else frames
    kind = "device" if isinstance(frames, StubDeviceFrames) else "be" if f.dtype == np.dtype(">f4") else "host"
    f = np.asarray(f, np.float32)
    return (f[None] if f.ndim == 2 else f), kind


class FakeContext:
    def __init__(self):
        self.calls = []                                   # (what, frames, where the frames were, flags that were set)

    def detect_batch(self, frames, params_bright, params_dim, cat=None, rs=None, pinned=False):
        f, kind = _host(frames)
        self.calls.append(("detect", len(f), kind, ("pinned",) if pinned else ()))
        assert cat is None or len(cat["count"]) == len(f)
        if len(f) > 1 and (f[:, 0, GROUP_FAIL] != 0).any():
            raise RuntimeError("the group call failed")
        rec = np.zeros(len(f), _native.RESULT_DTYPE)
        rec["found"], rec["status"] = f[:, 0, 0] > 0, f[:, 0, 1]
        rec["rho"], rec["theta"] = f[:, 1, 0], f[:, 1, 1]
        return rec

    def measure_trails(self, frames, records, cat=None, rs=None, pinned=False, native_device=False, **params):
        f, kind = _host(frames)
        self.calls.append(("measure", len(f), kind, tuple(n for n, v in (("pinned", pinned), ("native_device", native_device)) if v)))
        assert len(records) == len(f)
        if (f[:, 0, MEASURE_FAIL] != 0).any():
            raise RuntimeError("the measurement failed")
        trails = np.zeros(len(f), _native.TRAIL_DTYPE)
        trails["rho"], trails["theta"], trails["n_pos"] = records["rho"], records["theta"], records["found"]
        return trails, np.ascontiguousarray(f[:, 2, :5])

    def detects(self):
        return [c[1:] for c in self.calls if c[0] == "detect"]


class FakeSky:
    """stands in for _native.Sky: the records come from pixel [0, 4], the "normalised" frames are the input"""

    def __init__(self, ctx, shape, max_frames=None, **params):
        self.ctx, self.shape, self.max_frames, self._s, self.last = ctx, tuple(shape), max_frames, True, None

    def normalize(self, frames, out=None, meshes=False, pinned=False):
        f, _ = _host(frames)
        assert len(f) <= self.max_frames and f.shape[1:] == self.shape
        if out is not None:
            out[...] = f.reshape(out.shape)
        self.last = frames
        rec = np.zeros(len(f), _native.SKY_DTYPE)
        rec["sky"], rec["sigma"], rec["gain"] = f[:, 0, 4], 1.0, 1.0
        return rec

    def frames(self, n=None):
        return self.last

    def close(self):
        self._s = False


class Events:
    """one recording sink behind results, errors, profiles and sky: (file, text) in write order"""

    def __init__(self):
        self.log = []

    def file(self, name):
        ev = self

        class F:
            def write(self, text):
                ev.log.append((name, text))

            def flush(self):
                pass
        return F()

    def text(self, name):
        return "".join(t for n, t in self.log if n == name)

    def lines(self, name):
        return self.text(name).splitlines()


class RecordingTee(detecttrails._DefocusTee):
    """the defocus tee with its fit left out: what would be fitted is recorded in the shared sink"""

    def __init__(self, events):
        super().__init__(events.file("profiles"), None, {}, {})
        self.events = events

    def add(self, key, trail, profile):
        super().add(key, trail, profile)
        self.events.log.append(("defocus", "%s %s %s %s\n" % tuple(key)))


def entries(text):
    """errors text -> one string per entry, cut in front of every ids line"""
    return [e for e in re.split(r"(?m)^(?=\d+ \d+ [ugriz] \d+\n)", text) if e]


def heads_and_lasts(text):
    return [(e.splitlines()[0], e.rstrip("\n").splitlines()[-1]) for e in entries(text)]


def make_loaded(device=False):
    """A loader.Loaded of the tree's frames by hand, as FrameLoader.load leaves it."""
    out = loader.Loaded(KEYS)
    nslot = 1 + max(s for _, _, s in FRAMES if s is not None)
    buf, cats = np.zeros((nslot, *SHAPE), ">f4"), [None] * nslot
    for i, (item, (key, what, slot)) in enumerate(zip(detecttrails._load_many(KEYS), FRAMES)):
        if len(item) == 2:
            out.error[i] = item[1]
            continue
        _, img, _, cat = item
        out.hdr[i] = dict(HDR)
        if slot is None:
            out.array[i], out.cat[i] = img, cat
        else:
            out.slot[i], buf[slot], cats[slot] = slot, img, cat
    out.shape, out.cats = SHAPE, pack_catalogs(cats)
    if device:
        out.device = StubDeviceFrames(buf)
    else:
        out.buffer = buf
    return out


class Run:
    pass


@pytest.fixture
def drive(monkeypatch):
    """drive(which, profiles, sky, device) -> what the driver wrote and what it called"""
    def drive(which, profiles=False, sky=False, device=False):
        r = Run()
        r.ctx, r.uses, r.ev = FakeContext(), [], Events()

        @contextlib.contextmanager
        def use_context(h, w, inflight=None):
            r.uses.append((h, w, inflight))
            yield r.ctx
        monkeypatch.setattr(detecttrails, "use_context", use_context)
        monkeypatch.setattr(_native, "Sky", FakeSky)
        pb, pd, prs = default_params()
        kw = {}
        if profiles == "tee":
            kw.update(profiles=RecordingTee(r.ev), trail_params={})
        elif profiles:
            kw.update(profiles=detecttrails._DefocusTee(r.ev.file("profiles"), None, {}, {}), trail_params={})
        if sky:
            kw["sky"] = detecttrails._SkyStage(r.ev.file("sky"), None)
        res, err = r.ev.file("results"), r.ev.file("errors")
        if which == "field":
            for key in KEYS:
                detecttrails.process_field(res, err, *key, pb, pd, prs, **kw)
        elif which == "loaded":
            detecttrails.process_loaded(res, err, make_loaded(device), pb, pd, prs, **kw)
        else:
            detecttrails.process_fields_batched(res, err, KEYS, pb, pd, prs, **kw)
        r.results, r.profiles, r.sky, r.errors = r.ev.lines("results"), r.ev.lines("profiles"), r.ev.lines("sky"), r.ev.text("errors")
        return r
    return drive


def _key_of(line):
    return tuple(line.split()[:4])


def _skeys(keys):
    return [tuple(str(x) for x in k) for k in keys]


WANT_ERRORS = [("94 1 r 102", "'NoneType' object is not subscriptable"),
               ("94 1 r 103", "liblfdmi error %d: frame failed on the device" % _native.ERR_CAPACITY),
               ("94 1 r 104", None)]                      # (the missing file's message holds its path)


def _check_plain_rows(r, profiles):
    assert [_key_of(ln) for ln in r.results] == _skeys(DETECTED)
    assert all(len(ln.split()) == 17 for ln in r.results)
    assert [_key_of(ln) for ln in r.profiles] == (_skeys(DETECTED) if profiles else [])
    got = heads_and_lasts(r.errors)
    assert [h for h, _ in got] == [h for h, _ in WANT_ERRORS]
    assert all(w is None or w == g for (_, g), (_, w) in zip(got, WANT_ERRORS))
    assert "FileNotFoundError" in entries(r.errors)[2]
    for e in entries(r.errors):
        assert e.endswith("\n\n") and e.count("\n\n") == 1


@pytest.mark.parametrize("profiles", [False, True, "tee"])
def test_loaded_batched_and_frame_by_frame_write_the_same(tree, drive, profiles):
    """the three drivers over the same frames: the same results and profiles rows, errors entries with the same heads and messages"""
    tree()
    runs = {which: drive(which, profiles) for which in ("loaded", "batched", "field")}
    for r in runs.values():
        _check_plain_rows(r, profiles)
        assert r.results == runs["loaded"].results and r.profiles == runs["loaded"].profiles
        assert heads_and_lasts(r.errors) == heads_and_lasts(runs["loaded"].errors)
        if profiles == "tee":                             # every profiles row is handed to the fit, after it was written
            assert [n for n, _ in r.ev.log if n in ("profiles", "defocus")] == ["profiles", "defocus"] * len(DETECTED)
            assert [tuple(t.split()) for n, t in r.ev.log if n == "defocus"] == _skeys(DETECTED)
    # one call per run of neighbouring same-filter slots, from pinned memory; the other frame on its own from a host array
    ld = runs["loaded"]
    assert ld.ctx.detects() == [(5, "be", ("pinned",)), (1, "be", ("pinned",)), (1, "host", ())]
    assert [u for u in ld.uses if u[2] is not None] == [(8, 9, 5), (8, 9, 1)]
    if profiles:
        assert [c for c in ld.ctx.calls if c[0] == "measure"] == [("measure", 5, "be", ("pinned",)), ("measure", 1, "be", ("pinned",)),
                                                                  ("measure", 1, "host", ())]
    # one call per (filter, shape) group of stacked host frames
    bt = runs["batched"]
    assert sorted(bt.ctx.detects()) == [(1, "host", ()), (1, "host", ()), (5, "host", ())]
    assert sorted(u for u in bt.uses if u[2] is not None) == [(7, 9, 1), (8, 9, 1), (8, 9, 5)]
    assert runs["field"].ctx.detects() == [(1, "host", ())] * 7


def test_device_chunk_takes_the_device_frames(tree, drive):
    tree()
    r = drive("loaded", True, device=True)
    _check_plain_rows(r, True)
    assert r.ctx.calls[:4] == [("detect", 5, "device", ()), ("measure", 5, "device", ("native_device",)),
                               ("detect", 1, "device", ()), ("measure", 1, "device", ("native_device",))]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("profiles", [False, True])
def test_sky_rows_come_first(tree, drive, profiles, device):
    """a frame's sky row is written ahead of its results row or errors entry; the frame whose file is missing has none"""
    tree()
    runs = {which: drive(which, profiles, sky=True, device=device) for which in (("loaded",) if device else ("loaded", "field"))}
    for r in runs.values():
        _check_plain_rows(r, profiles)
        assert [_key_of(ln) for ln in r.sky] == _skeys(k for k, what, _ in FRAMES if what != "missing")
        assert [float(ln.split()[5]) for ln in r.sky] == [100.0 + j for j, f in enumerate(FRAMES) if f[1] != "missing"]
        order = []
        for name, text in r.ev.log:                       # every file's rows, frame by frame, in write order
            if name == "sky" or name == "results" or (name == "errors" and re.match(r"\d+ \d+ [ugriz] \d+\n$", text)):
                order.append((name, _key_of(text)))
        want = []
        for key, what, _ in FRAMES:
            want += [("sky", _skeys([key])[0])] if what != "missing" else []
            want += [("results" if what in ("detected", "array") else "errors", _skeys([key])[0])] if what != "undetected" else []
        assert order == want
        assert r.results == runs["loaded"].results and r.profiles == runs["loaded"].profiles
    # detection and measurement read the sky handle's buffer: no flags
    ld = runs["loaded"]
    assert ld.ctx.detects()[:2] == [(5, "device" if device else "be", ()), (1, "device" if device else "be", ())]
    assert all(c[3] == () for c in ld.ctx.calls)


@pytest.fixture
def group_failure(tree, drive):
    """one frame of the r run fails every call that holds more than one frame"""
    tree({(94, 1, "r", 101): (GROUP_FAIL,)})
    return {(which, sky): drive(which, True, sky=sky) for which in ("loaded", "batched") for sky in (False, True) if which == "loaded" or not sky}


def test_failed_group_call_goes_frame_by_frame(group_failure):
    for (which, sky), r in group_failure.items():
        assert [_key_of(ln) for ln in r.results] == _skeys(DETECTED)
        assert [_key_of(ln) for ln in r.profiles] == _skeys(DETECTED)
        got = heads_and_lasts(r.errors)
        assert [h for h, _ in got] == [h for h, _ in WANT_ERRORS] and [g for _, g in got[:2]] == [w for _, w in WANT_ERRORS[:2]]
        if sky:
            assert [_key_of(ln) for ln in r.sky] == _skeys(k for k, what, _ in FRAMES if what != "missing")
    ld = group_failure["loaded", False]
    assert ld.ctx.detects() == [(5, "be", ("pinned",))] + [(1, "host", ())] * 5 + [(1, "be", ("pinned",)), (1, "host", ())]
    assert sorted(group_failure["batched", False].ctx.detects()) == [(1, "host", ())] * 7 + [(5, "host", ())]


def test_fallback_entries_are_one_block(group_failure):
    """a frame that fails on its own after a failed group call logs one entry that ends in one blank line, like frame by frame"""
    for r in group_failure.values():
        found = entries(r.errors)
        assert len(found) == 3
        for e in found:
            assert e.endswith("\n\n") and e.count("\n\n") == 1
            assert "During handling" not in e and "the group call failed" not in e


@pytest.mark.parametrize("which", ["loaded", "batched"])
def test_failed_group_measurement_is_every_detected_frames_error(tree, drive, which):
    """the r run's measure_trails raises: its detected frames keep their results rows and log the measurement's message"""
    tree({(94, 1, "r", 101): (MEASURE_FAIL,)})
    r = drive(which, True)
    hit = _skeys([(94, 1, "r", 100), (94, 1, "r", 106)])
    assert [_key_of(ln) for ln in r.results] == _skeys(DETECTED)
    assert [_key_of(ln) for ln in r.profiles] == [k for k in _skeys(DETECTED) if k not in hit]
    got = heads_and_lasts(r.errors)
    assert [g for g in got if g[1] == "the measurement failed"] == [(" ".join(k), "the measurement failed") for k in hit]
    assert len(got) == len(WANT_ERRORS) + 2
    rows = [(n, _key_of(t)) for n, t in r.ev.log if n == "results" or (n == "errors" and re.match(r"\d+ \d+ [ugriz] \d+\n$", t))]
    for k in hit:                                         # the results row first, then the entry
        assert rows.index(("results", k)) + 1 == rows.index(("errors", k))


@pytest.mark.parametrize("sky", [False, True])
def test_failed_call_on_a_device_chunk_is_every_frames_error(tree, drive, sky):
    """a device chunk whose call fails: the frames are wherever the failed call left them: no second source, no single-frame call"""
    tree({(94, 1, "r", 101): (GROUP_FAIL,)})
    r = drive("loaded", True, sky=sky, device=True)
    run = [k for k, _, slot in FRAMES if slot is not None and slot < 5]
    got = dict(heads_and_lasts(r.errors))
    assert all(got[" ".join(str(x) for x in k)] == "the group call failed" for k in run)
    assert [_key_of(ln) for ln in r.results] == _skeys([(94, 1, "g", 100), (94, 1, "r", 105)])
    assert r.ctx.detects() == [(5, "device", ()), (1, "device", ()), (1, "host", ())]
    if sky:                                               # normalised before the call failed: the rows are there
        assert [_key_of(ln) for ln in r.sky] == _skeys(k for k, what, _ in FRAMES if what != "missing")
    for e in entries(r.errors):
        assert e.endswith("\n\n") and e.count("\n\n") == 1


def test_a_loaded_built_by_hand_has_its_catalogue_slot():
    out = loader.Loaded([(94, 1, "r", 100)])
    assert out.cats is None and out.cat_of(0) is None
