"""What the variable-diagonal fine level (k_zsweep_rb7<...,VD>, k_zresrestrict<7,...,VD>) gains
over the field kernels it replaces, against the parent commit's library.

Prior: 3D ShiftedLaplaceFDOperator with PeriodicCorrelationLengthModel(0.2, 0.4), f = 0, one chain.  One process
assembles the matrix once and creates one sampler per library on it -- the parent's (build/libmgmc_parent.so:
the parent commit's multigridmc_amd/csrc and include compiled with the product's flags, the recipe of DESIGN.md
section 8 "Parent against head") and the head's -- same seed, same state.  Then `rounds` rounds alternate
parent, head, parent, head, ...: per run
8 untimed cycles, `cycles` cycles timed with sample_timed (HIP events on the handle's stream, first to last
event) and `nsweeps` fine sweeps timed by mgmc_time_fine_sweeps (on scratch copies: the chain is not advanced).
Both samplers run the same cycles, so their final states must be the same bytes: a SHA-256 of each is recorded
and compared.  The yardstick is the parent, never MGMC_DISABLE=zsweep of the head.

    python scripts/vardiag_cost.py [--size 256:6] [--cycles N] [--rounds R] [--nsweeps S]
                                   [--parent build/libmgmc_parent.so] [--out profiles/vardiag/cost.json]

Per-kernel times come from a kernel trace, taken in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python scripts/vardiag_cost.py --trace-run 256:6 [--library LIB]
runs 8 cycles on one library and nothing else.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 5418513


def load(path):
    """libmgmc of `path` with every symbol it has bound (an older library lacks the newer entries)."""
    from multigridmc_amd import _native
    lib = ctypes.CDLL(path)
    for name, res, args in _native.SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    if lib.mgmc_abi_version() != _native.ABI_VERSION:
        raise ImportError(f"{path}: ABI {lib.mgmc_abi_version()}, this package needs {_native.ABI_VERSION}")
    return lib


def make_sampler(mg, lib, op, nlevel):
    """a MultigridMCSampler on `lib` (the package binds its samplers to the library loaded at their creation)"""
    from multigridmc_amd import _native
    _native._lib = lib
    return mg.MultigridMCSampler(op, SEED, mg.MultigridParameters(nlevel=nlevel))


def digest(s):
    return hashlib.sha256(s.get_state().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256:6", help="N:NLEVEL, an N^3 lattice")
    ap.add_argument("--cycles", type=int, default=0, help="cycles per timed window (0: by size)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--nsweeps", type=int, default=20)
    ap.add_argument("--parent", default=os.path.join(ROOT, "build", "libmgmc_parent.so"))
    ap.add_argument("--head", default=os.path.join(ROOT, "multigridmc_amd", "libmgmc_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vardiag", "cost.json"))
    ap.add_argument("--trace-run", default="", help="N:NLEVEL -- 8 cycles on --library only (for a kernel trace)")
    ap.add_argument("--library", default="", help="--trace-run: the library (default: the head's)")
    a = ap.parse_args()
    import multigridmc_amd as mg

    n, nlevel = (int(v) for v in (a.trace_run or a.size).split(":"))
    t0 = time.time()
    op = mg.ShiftedLaplaceFDOperator(mg.Lattice3d(n, n, n), mg.PeriodicCorrelationLengthModel(0.2, 0.4))
    op.get_csr()
    t_csr = time.time() - t0
    print(f"{n}^3: matrix assembled in {t_csr:.1f} s", flush=True)
    if a.trace_run:
        s = make_sampler(mg, load(a.library or a.head), op, nlevel)
        s.sample(8)
        print(f"{n}^3 / {nlevel} levels on {a.library or a.head}: {s.level_kernels(0)}; state {digest(s)}")
        s.close()
        return

    libs = (("parent", a.parent), ("head", a.head))
    samplers, setup_s = {}, {}
    for name, path in libs:
        t0 = time.time()
        samplers[name] = make_sampler(mg, load(path), op, nlevel)
        setup_s[name] = time.time() - t0
        print(f"{name}: created in {setup_s[name]:.1f} s; level 0 {samplers[name].level_kernels(0)}", flush=True)
    cycles = a.cycles or (40 if n >= 256 else 200)
    runs = []
    for r in range(a.rounds):
        for name, _ in libs:
            s = samplers[name]
            s.sample(8)
            cycle_ms = s.sample_timed(cycles, stride=cycles)["total_ms"] / cycles
            sweep_ms = s.time_fine_sweeps(a.nsweeps) / a.nsweeps
            runs.append({"round": r, "library": name, "cycle_ms": cycle_ms, "fine_sweep_ms": sweep_ms})
            print(f"round {r} {name:6s}: cycle {cycle_ms:.4f} ms, fine sweep {sweep_ms:.4f} ms", flush=True)
    out = {"lattice": [n, n, n], "nlevel": nlevel, "prior": "fd, PeriodicCorrelationLengthModel(0.2, 0.4)",
           "cycles_per_run": cycles, "sweeps_per_run": a.nsweeps, "rounds": a.rounds, "assemble_s": t_csr,
           "create_s": setup_s, "runs": runs, "libraries": {}}
    for name, path in libs:
        s = samplers[name]
        mine = [q for q in runs if q["library"] == name]
        entry = {"path": os.path.relpath(path, ROOT), "level0": s.level_kernels(0), "state_sha256": digest(s)}
        for key in ("cycle_ms", "fine_sweep_ms"):
            v = [q[key] for q in mine]
            entry[key] = {"median": statistics.median(v), "min": min(v), "max": max(v),
                          "spread": (max(v) - min(v)) / statistics.median(v)}
        out["libraries"][name] = entry
        s.close()
    p, h = out["libraries"]["parent"], out["libraries"]["head"]
    out["states_identical"] = p["state_sha256"] == h["state_sha256"]
    out["cycle_ratio_parent_over_head"] = p["cycle_ms"]["median"] / h["cycle_ms"]["median"]
    out["fine_sweep_ratio_parent_over_head"] = p["fine_sweep_ms"]["median"] / h["fine_sweep_ms"]["median"]
    # faster by more than the parent's own spread: the head's slowest run against the parent's fastest
    out["head_faster_beyond_parent_spread"] = {key: h[key]["max"] < p[key]["min"] for key in ("cycle_ms", "fine_sweep_ms")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"cycle {p['cycle_ms']['median']:.4f} -> {h['cycle_ms']['median']:.4f} ms "
          f"(x{out['cycle_ratio_parent_over_head']:.2f}), fine sweep {p['fine_sweep_ms']['median']:.4f} -> "
          f"{h['fine_sweep_ms']['median']:.4f} ms (x{out['fine_sweep_ratio_parent_over_head']:.2f}); parent spread "
          f"{100 * p['cycle_ms']['spread']:.1f}% / {100 * p['fine_sweep_ms']['spread']:.1f}%; states identical: "
          f"{out['states_identical']}")
    print(f"wrote {a.out}")
    if not out["states_identical"]:
        sys.exit("the two libraries' final states differ")


if __name__ == "__main__":
    main()
