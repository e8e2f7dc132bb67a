"""Child process of tests/test_gpu_tuning.py (a helper like tests/cpp_client.py; pytest does not collect it).

    MGMC_LIBRARY=<library> python tests/tuning_worker.py <cases.json>

Runs every case of the file in order through the library MGMC_LIBRARY names and compares each result with the
arrays the parent computed with the CPU oracle (np.array_equal against the .npy files the case lists).  Prints one
JSON line per case:

    {"id": ..., "ok": true | false, "labels": [level_kernels(0), ...], "checks": <number of comparisons>,
     "mismatches": [{"what": ..., "count": n, "first": [i, j, k], "last": [i, j, k]}, ...], "error": text | null,
     "seconds": t}

and a first line {"num_cu": ...} with the compute units the device reports.  MGMC_DISABLE and MGMC_POISON are read
per handle, so they are set here before each mgmc_create.  A HIP error ends the run (exit status 3): nothing more
is started on a device that reported one.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import multigridmc_amd as mg  # noqa: E402
from multigridmc_amd import _native  # noqa: E402

SEED = 5418513
KAPPA_SQ = 25.0
HIP_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63  # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


def num_cu():
    hip = ctypes.CDLL("libamdhip64.so")
    v = ctypes.c_int(0)
    rc = hip.hipDeviceGetAttribute(ctypes.byref(v), HIP_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0)
    return v.value if rc == 0 else -1


class Checker:
    def __init__(self, case):
        self.case = case
        self.nchecks = 0
        self.mismatches = []

    def expected(self, key):
        return np.load(os.path.join(self.case["dir"], key + ".npy"))

    def check(self, key, got, shape=None):
        """got against <dir>/<key>.npy; shape: the lattice whose interior vertices the vector holds (None: a
        series, reported by index)."""
        want = self.expected(key)
        got = np.asarray(got, dtype=np.float64)
        self.nchecks += 1
        if got.shape == want.shape and np.array_equal(got, want):
            return
        if got.shape != want.shape:
            self.mismatches.append({"what": key, "count": -1, "first": list(got.shape), "last": list(want.shape)})
            return
        per = int(np.prod([n - 1 for n in shape])) if shape else got.shape[-1]
        bad = np.flatnonzero(~((got == want).reshape(-1)))
        lat = mg.Lattice(*shape) if shape else None

        def where(q):  # (chain, i, j, k) of a flat index
            c, ell = divmod(int(q), per)
            at = list(lat.vertexidx_linear2euclidean(ell)) if lat else [ell]
            return ([c] if got.ndim > 1 else []) + at

        self.mismatches.append({"what": key, "count": int(bad.size), "first": where(bad[0]), "last": where(bad[-1])})


def parameters(case):
    return mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **case["params"]})


def make_sampler(case):
    for key, value in (("MGMC_DISABLE", case["disable"]), ("MGMC_POISON", "1" if case["poison"] else "")):
        if value:
            os.environ[key] = value
        else:
            os.environ.pop(key, None)
    lat = mg.Lattice(*case["shape"])
    if case.get("operator"):  # a matrix handle with a variable-diagonal fine level: "fd_periodic" | "dominant"
        from tests.test_gpu_vardiag import build_operator
        assert case["operator"] in ("fd_periodic", "dominant") and case["measurements"] is None
        op, lat = build_operator(tuple(case["shape"]), case["operator"] == "dominant", case.get("lowrank", False))
    elif case["measurements"] is not None:
        from tests.test_gpu_lowrank import measured
        op, lat = measured(tuple(case["shape"]), KAPPA_SQ, *case["measurements"])
    else:
        op = mg.ShiftedLaplaceFDOperator(lat, KAPPA_SQ)
    s = mg.MultigridMCSampler(op, SEED, parameters(case), device=0, chain_id=case["chain0"], nchains=case["nchains"])
    return s, lat


def run_cycles(case, s, lat, chk):
    """Two cycles with a random right-hand side from the zero state, then four cycles of the prior (f = 0) from the
    zero state with the QoI series, every chain."""
    n = lat.Nvertex
    k = case["nchains"]
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    f = np.random.default_rng(7).standard_normal(n)
    if k == 1:
        x = np.zeros(n)
        for cycle in (1, 2):
            s.apply(f, x)
            chk.check(f"apply{cycle}", x[None, :], lat.shape)
    else:  # a batch: the device-resident loop (apply moves one chain's state)
        s.fix_rhs(f)
        s.set_state(np.zeros(n))
        s.sample(2)
        chk.check("apply2", s.get_state(None), lat.shape)
    zero = np.zeros(n)
    s.fix_rhs(zero)
    s.set_state(zero)
    z = s.sample(4, qoi, chain=None if k > 1 else 0)
    chk.check("prior_series", np.reshape(z, (k, 4)))
    chk.check("prior_state", s.get_state(None), lat.shape)


def run_sweeps(case, s, chk):
    """The component calls on every level (tests/test_gpu_parity.py test_multicolour_sweeps_bitwise, and the
    residual + restriction): a cycle mismatch is then attributed to a kernel."""
    p = parameters(case)
    rng = np.random.default_rng(7)
    for level in range(p.nlevel):
        d = s.level_desc(level)
        b = rng.standard_normal(d["ndof"])
        x = rng.standard_normal(d["ndof"])
        for direction in (mg.FORWARD, mg.BACKWARD):
            chk.check(f"smoother_l{level}_d{direction}", s.smoother_apply(level, direction, 2, b, x), d["shape"])
            chk.check(f"sampler_l{level}_d{direction}", s.sor_sampler_apply(level, direction, 5 + level, 77, b, x),
                      d["shape"])
        if level + 1 < p.nlevel:
            chk.check(f"residual_restrict_l{level}", s.residual_restrict(level, b, x),
                      s.level_desc(level + 1)["shape"])


def run_field_stats(case, s, lat, chk):
    s.field_stats()
    s.sample(case["field_stats"])
    n, mean, m2 = s.field_moments()
    chk.check("fs_count", np.array([float(n)]))
    chk.check("fs_mean", mean, lat.shape)
    chk.check("fs_m2", m2, lat.shape)


def run_case(case):
    chk = Checker(case)
    out = {"id": case["id"], "ok": False, "labels": None, "checks": 0, "mismatches": [], "error": None}
    t0 = time.perf_counter()
    s = None
    try:
        s, lat = make_sampler(case)
        if case["field_stats"]:
            run_field_stats(case, s, lat, chk)
        else:
            run_cycles(case, s, lat, chk)
            if case["sweeps"]:
                run_sweeps(case, s, chk)
        # (after the prior run: level 0 carries rhs=zero where the cycle ran the zero-right-hand-side instances)
        out["labels"] = [s.level_kernels(level) for level in range(parameters(case).nlevel)]
        s.close()
    except mg.MgmcError as e:
        out["error"] = str(e)
        out["hip_error"] = e.code == _native.MGMC_E_HIP
    out["checks"] = chk.nchecks
    out["mismatches"] = chk.mismatches
    out["ok"] = out["error"] is None and not chk.mismatches and chk.nchecks > 0
    out["seconds"] = round(time.perf_counter() - t0, 3)
    return out


def main(argv):
    with open(argv[1]) as fh:
        cases = json.load(fh)
    mg.load_library()
    print(json.dumps({"num_cu": num_cu(), "library": os.environ.get("MGMC_LIBRARY", _native.LIB_PATH)}), flush=True)
    for case in cases:
        out = run_case(case)
        print(json.dumps(out), flush=True)
        if out.get("hip_error"):
            return 3
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
