"""Child of tests/test_gpu_rs_routes.py: LFDMI_PREP_ROWS and LFDMI_RS_FILL_FRAC are read once per process, so the parent sets them
for a fresh interpreter.  argv[1]: an .npz with, per case name, the reference's ERODED / CANNY / BOX images, the literal frame,
the oracle's record (JSON) and its count of accepted rectangles.  Every case runs lfdmi_detect_batch with its catalogue on
device and on host frames, stage images off.  Exit status 0: every case equal."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import torch
    import front_cases as fc
    import rs_cases as R
    from lfd_amd import _native
    from lfd_amd.catalogs import pack_catalogs
    assert "LFDMI_PREP_ROWS" in os.environ or "LFDMI_RS_FILL_FRAC" in os.environ
    ref = np.load(sys.argv[1])
    names = sorted(k[8:] for k in ref.files if k.startswith("literal_"))
    ids = dict(ERODED=_native.STAGE_ERODED, CANNY=_native.STAGE_CANNY, BOX=_native.STAGE_BOX)
    pb, pd = R.dim_params()
    bad = []
    for name in names:
        c = R.BY_NAME[name]
        rs = _native.make_rs_params(c.filter, **c.kw)
        want_rec = json.loads(str(ref["record_" + name]))
        ok = True
        for dev in (True, False):
            with _native.Context(0, c.h, c.w, 1) as ctx:
                ctx.set_stage_images(0)
                frames = torch.from_numpy(np.array(c.frame[None])).cuda() if dev else np.array(c.frame[None])
                rec = ctx.detect_batch(frames, pb, pd, pack_catalogs([c.cat]), rs)
                if dev:
                    torch.cuda.synchronize()
                back = frames.cpu().numpy() if dev else frames
                ok = ok and np.array_equal(back[0].view(np.uint32), ref["literal_" + name].view(np.uint32))
                ok = ok and all(rec[0][k].item() == v for k, v in want_rec.items())
                ok = ok and int(ctx.get_counters(0, 1)[0, fc.C_NQUADS]) == int(ref["nboxes_" + name])
                for st, sid in ids.items():
                    got, want = ctx.get_stage(0, sid, c.h, c.w), ref[f"{st}_{name}"]
                    if st != "ERODED":
                        got, want = got != 0, want != 0
                    same = np.array_equal(got, want)
                    if not same:
                        print(f"{name}: {'device' if dev else 'host'} frames: stage {st}: {int((got != want).sum())} pixels differ, first at "
                              f"{tuple(int(v) for v in np.argwhere(got != want)[0])}", flush=True)
                    ok = ok and same
        print(name, "ok" if ok else "DIFFERS", flush=True)
        if not ok:
            bad.append(name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
