"""Child process of tests/test_gpu_field_batch.py (a helper like tests/tuning_worker.py; pytest does not collect it).

    python tests/field_batch_worker.py <library> <case> <batch> <ncycles>

Loads the library by path, runs the bitwise case of the batch-means field statistics through it -- a handle with
field_stats(1, batch) samples ncycles cycles at once, a twin handle of the same library is stepped one cycle at a
time into the numpy mirror -- and prints one JSON line
    {"ok": bool, "nb": completed batches, "fields": [names of the fields that differ], "error": text | null}.
A HIP error ends the run with exit status 3.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import multigridmc_amd as mg  # noqa: E402
from multigridmc_amd import _native  # noqa: E402


def main(argv):
    path, name, batch, ncycles = argv[1], argv[2], int(argv[3]), int(argv[4])
    _native._lib = mg.load_library(path)  # (the package binds its samplers to the library loaded at their creation)
    from tests.test_field_batch_host import BatchMirror
    from tests.test_gpu_field_batch import make, mirror_cycles
    out = {"ok": False, "nb": 0, "fields": [], "error": None, "library": path}
    try:
        a, b = make(name), make(name)
        a.field_stats(1, batch=batch)
        a.sample(ncycles)
        m = BatchMirror(b.ndof, b.nchains, batch)
        mirror_cycles(b, m, ncycles, 0, 1)
        nb, bmean, bm2 = a.field_batch_moments()
        n, mean, m2 = a.field_moments()
        got = {"bmean": bmean, "bm2": bm2, "mean": mean, "m2": m2}
        want = {"bmean": m.bmean, "bm2": m.bm2, "mean": m.mean, "m2": m.m2}
        out["nb"] = int(nb)
        out["fields"] = [k for k in got if not np.array_equal(got[k], want[k])]
        out["ok"] = nb == m.nb and n == m.n and not out["fields"] and bool(np.any(bm2 > 0))
        a.close()
        b.close()
    except mg.MgmcError as e:
        out["error"] = str(e)
        print(json.dumps(out), flush=True)
        return 3 if e.code == _native.MGMC_E_HIP else 1
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
