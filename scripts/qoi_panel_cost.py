"""What recording a QoI panel (MultigridMCSampler.qoi_panel_record, mgmc_panel.hpp) adds to a cycle, next to the
parent commit's library.  Modelled on scripts/energy_cost.py.

On one lattice (default 3D 256^3 / 6 levels, the prior with f = 0) one process holds two samplers on the parent's
library (build/libmgmc_parent.so, DESIGN.md section 8 "Parent against head") and one on the head's, and runs these
variants interleaved, round by round, in an order that alternates between rounds (the order of
creation and of running moves a cycle time by up to 1 %):

    parent_off, parent2_off    the parent's library, two samplers of its own
    off                        the head's library, no panel
    config5p                   ... recording the 9 columns of config 5': 8 ball averages (radius 0.05) and the global
                               average (a dense constant column)
    dense8                     ... recording 8 dense columns with distinct values
    dense8_g1                  (with --ungrouped LIB) the same panel on a build of the head with QP_G = 1 in
                               mgmc_panel.hpp: one wavefront per (dense column, block), 16 bytes per unknown and
                               column; its added time is taken against "off" of the head

A round of a variant is `cycles` cycles timed with sample_timed after 16 untimed cycles of the variant.  All samplers
run the same number of cycles in all and their final states are compared bit for bit.  Per variant: the median, the
extremes and the spread of the cycle time over the rounds; for the two panels the time added against "off", the
bytes of the model -- 8 (D + ceil(D / QP_G)) per unknown for D dense columns with values, 8 ceil(D_c / QP_G) more
for the D_c constant ones' share of x, 24 per entry of an entry-list column (offset, value, x) -- and the ratio of
the added time to those bytes at the 6.0 TB/s stream ceiling (profiles/r01_stream_ceiling.txt).  No threshold: the
script reports; exit status 2 only if the final states differ.

    python scripts/qoi_panel_cost.py [--size 256:6] [--cycles N] [--rounds R]
                                     [--parent build/libmgmc_parent.so] [--ungrouped build/libmgmc_panel_g1.so]
                                     [--out profiles/qoi_panel/cost.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from energy_cost import SEED, STREAM_CEILING, load, make  # noqa: E402

QP_G = 8  # mgmc_panel.hpp
VARIANTS = (("parent_off", "parent", None), ("parent2_off", "parent2", None), ("off", "head", None),
            ("config5p", "head", "config5p"), ("dense8", "head", "dense8"))


def panels(mg, n):
    lat = mg.Lattice3d(n, n, n)
    post = mg.synthetic_posterior(mg.ShiftedLaplaceFDOperator(lat, 25.0), 8, 0.05, True)
    rng = np.random.default_rng(20250219)
    rows = np.arange(lat.Nvertex, dtype=np.int64)
    return {"config5p": mg.measurement_panel(post), "dense8": [(rows, rng.standard_normal(lat.Nvertex)) for _ in range(8)]}


def model_bytes(cols, N):
    dense = [c for c in cols if len(c[0]) == N]
    const = [c for c in dense if np.all(c[1] == c[1][0])]
    nv = len(dense) - len(const)
    groups = -(-len(dense) // QP_G)
    return 8 * N * (nv + groups) + 24 * sum(len(c[0]) for c in cols if len(c[0]) != N)


def measure(mg, libs, n, nlevel, cycles, rounds):
    global VARIANTS
    if "g1" in libs:
        VARIANTS = VARIANTS + (("dense8_g1", "g1", "dense8"),)
    samplers = {name: make(mg, lib, n, nlevel) for name, lib in libs.items()}
    cols = panels(mg, n)
    N = samplers["head"].ndof
    for s in samplers.values():
        s.sample(16)
    times = {v[0]: [] for v in VARIANTS}
    head = samplers["head"]
    for r in range(rounds):
        order = VARIANTS if r % 2 == 0 else VARIANTS[::-1]
        for name, which, panel in order:
            s = samplers[which]
            if which == "head":
                s.set_qoi_panel(cols[panel] if panel else None)
                if panel:
                    s.qoi_panel_record(1, 32, 64)
            elif which == "g1" and r == 0:  # (its one variant: installed once)
                s.set_qoi_panel(cols[panel])
                s.qoi_panel_record(1, 32, 64)
            s.sample(16)
            times[name].append(s.sample_timed(cycles, stride=cycles)["total_ms"] / cycles)
        for k in ("parent", "parent2", "g1"):  # catch up with the head's three variants
            if k in samplers:
                samplers[k].sample(2 * (16 + cycles))
        print(f"  round {r}: " + ", ".join(f"{name} {times[name][-1]:.4f}" for name, _, _ in VARIANTS), flush=True)
    head.set_qoi_panel(None)
    head_state = head.get_state()
    same = bool(all(np.array_equal(s.get_state(), head_state) for s in samplers.values()))
    index = [samplers[k].get_sample_index() for k in ("parent", "parent2", "head")]
    for s in samplers.values():
        s.close()
    out = {"lattice": [n, n, n], "nlevel": nlevel, "ndof": N, "cycles_per_round": cycles, "rounds": rounds,
           "sample_index": index, "final_states_identical": same, "group_width": QP_G, "variants": {}}
    v = out["variants"]
    for name, which, panel in VARIANTS:
        t = times[name]
        med = statistics.median(t)
        v[name] = {"library": which, "cycle_ms_median": med, "cycle_ms_min": min(t), "cycle_ms_max": max(t),
                   "spread": (max(t) - min(t)) / med, "cycle_ms_rounds": t}
    for name, which, panel in VARIANTS:
        if panel is None:
            continue
        e, off = v[name], v["off"]["cycle_ms_median"]
        e["columns"] = len(cols[panel])
        e["added_ms_per_cycle"] = e["cycle_ms_median"] - off
        e["added_fraction_of_cycle"] = e["added_ms_per_cycle"] / off
        e["model_bytes"] = model_bytes(cols[panel], N) if which == "head" else 16 * N * len(cols[panel])
        e["model_ms_at_stream_ceiling"] = e["model_bytes"] / STREAM_CEILING * 1e3
        e["added_over_model"] = e["added_ms_per_cycle"] / e["model_ms_at_stream_ceiling"]
    p = v["parent_off"]
    out["agrees_with_parent"] = {
        "head_median": v["off"]["cycle_ms_median"], "parent_median": p["cycle_ms_median"],
        "parent_min": p["cycle_ms_min"], "parent_max": p["cycle_ms_max"],
        "parent2_median": v["parent2_off"]["cycle_ms_median"],
        "head_over_parent": v["off"]["cycle_ms_median"] / p["cycle_ms_median"],
        "within_parent_spread": abs(v["off"]["cycle_ms_median"] - p["cycle_ms_median"])
        <= p["cycle_ms_max"] - p["cycle_ms_min"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256:6")
    ap.add_argument("--cycles", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--parent", default=os.path.join(ROOT, "build", "libmgmc_parent.so"))
    ap.add_argument("--ungrouped", default="", help="a build of the head with QP_G = 1 (adds the dense8_g1 variant)")
    ap.add_argument("--head", default=os.path.join(ROOT, "multigridmc_amd", "libmgmc_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qoi_panel", "cost.json"))
    a = ap.parse_args()
    import multigridmc_amd as mg
    libs = {"parent": load(a.parent), "head": load(a.head)}
    libs["parent2"] = libs["parent"]
    if a.ungrouped:
        libs["g1"] = load(a.ungrouped)
    n, nlevel = (int(v) for v in a.size.split(":"))
    print(f"{n}^3 / {nlevel} levels, {a.cycles} cycles per window:", flush=True)
    r = measure(mg, libs, n, nlevel, a.cycles, a.rounds)
    v, g = r["variants"], r["agrees_with_parent"]
    for name in [k for k in v if "model_bytes" in v[k]]:
        e = v[name]
        print(f"  {name}: +{e['added_ms_per_cycle']:.4f} ms per recorded cycle ({100 * e['added_fraction_of_cycle']:.1f} % of "
              f"the cycle); model {e['model_bytes'] / 1e6:.1f} MB = {e['model_ms_at_stream_ceiling']:.4f} ms at the "
              f"stream ceiling: ratio {e['added_over_model']:.2f}")
    print(f"  off: head {g['head_median']:.4f} ms, parent {g['parent_median']:.4f} ms ({g['parent_min']:.4f} .. "
          f"{g['parent_max']:.4f}; its second sampler {g['parent2_median']:.4f}): "
          f"{'within' if g['within_parent_spread'] else 'OUTSIDE'} the parent's spread; final states identical: "
          f"{r['final_states_identical']}", flush=True)
    doc = {"parent_library": os.path.relpath(a.parent, ROOT), "stream_ceiling_bytes_per_s": STREAM_CEILING,
           "results": [r]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")
    if not r["final_states_identical"]:
        sys.exit(2)


if __name__ == "__main__":
    main()
