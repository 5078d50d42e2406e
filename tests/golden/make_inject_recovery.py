"""Writes tests/golden/inject_recovery.json and tests/golden/inject_plan.json: the rows of the 16-frame recovery set
(tests/inject_ref.py: recovery_set) injected with the numpy restatement and detected with the oracle, and the checksum of the
plan recovery.draw_trails draws for it.

    python tests/golden/make_inject_recovery.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))


def cpu_rows():
    import inject_ref
    from lfd_amd import _native, recovery
    from lfd_amd.detecttrails import default_params
    from oracle import lfd_oracle as O
    pb, pd, prs = default_params()
    rs = O.rs_params("r", **{k: v for k, v in prs.items() if k != "debug"})
    frames, cats, plan, table, step = inject_ref.recovery_set()
    inject_ref.inject(frames, recovery.to_inject(plan), table, step, 4)
    recs = np.zeros(len(frames), _native.RESULT_DTYPE)
    for i in range(len(frames)):
        for k, v in O.detect_frame(frames[i], pb, pd, cats[i], rs).items():
            recs[i][k] = v
    return recovery.make_rows(recs, plan, pb, pd, inject_ref.SET_SHAPE), plan


def main():
    import inject_ref
    from lfd_amd import recovery
    rows, plan = cpu_rows()
    with open(os.path.join(HERE, "inject_recovery.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_inject_recovery.py", "k": recovery.K_MATCH, "rows": inject_ref.rows_to_json(rows)}, f, indent=1)
    with open(os.path.join(HERE, "inject_plan.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_inject_recovery.py", "n_frames": len(plan), "shape": list(inject_ref.SET_SHAPE),
                   "seed": inject_ref.SET_SEED, "sha256": recovery.plan_checksum(plan)}, f, indent=1)
    print("found %d matched %d of %d" % ((rows["found"] != 0).sum(), rows["matched"].sum(), len(rows)))


if __name__ == "__main__":
    main()
