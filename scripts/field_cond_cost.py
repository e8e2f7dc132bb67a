"""What the Rao-Blackwellised field statistics (MultigridMCSampler.field_stats(conditional=True),
mgmc_fieldcond.hpp) add to a cycle, against plain field_stats(1) in the same run.

For each lattice (default 3D 256^3 / 6 levels and 512^3 / 7 levels, the prior with f = 0 and one chain: bench.py's
workload) one sampler runs four variants in one process, interleaved round by round: statistics off, plain
stride 1, conditional fused (the z-march), conditional forced two-pass.  A round of a variant is `cycles` cycles
timed with sample_timed -- HIP events on the handle's stream, total = first to last event -- after 8 untimed cycles
of the variant.  Reported per variant: the median and the spread of the cycle time over the rounds and the added
time per cycle against "off"; for the fused path also the byte model's target,
    plain's added time x (8 h + 32) / 40 x 1.15,
h the x-read amplification of the z-march's tile ((FC_TY + 2) / FC_TY x (FC_TZ + 2) / FC_TZ + 2 / 64, from the
constants of mgmc_fieldcond.hpp), and whether the fused path beat the forced two passes in this run.

    python scripts/field_cond_cost.py [--sizes 256:6,512:7] [--cycles N] [--rounds R]
                                      [--out profiles/field_stats/cond_cost.json]

The kernels' own times come from a kernel trace, taken in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/field_cond_cost.py --trace-run 512:7
runs 32 cycles of each recording variant and nothing else; scripts/kstats.py DIR/.../kt_kernel_trace.csv 32 lists
k_fieldstats, k_fieldcond_z, k_operator_apply and k_fieldcond_c.
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> field_stats arguments (None: statistics off)
VARIANTS = (("off", None), ("plain", {}), ("cond_fused", {"conditional": True}),
            ("cond_two_pass", {"conditional": True, "two_pass": True}))


def tile_constants():
    text = open(os.path.join(ROOT, "multigridmc_amd", "csrc", "mgmc_fieldcond.hpp")).read()
    return {k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("FC_XP", "FC_TY", "FC_TZ")}


def x_amplification(c):
    return (c["FC_TY"] + 2) / c["FC_TY"] * (c["FC_TZ"] + 2) / c["FC_TZ"] + 2 / (2 * c["FC_XP"])


def enable(s, kw):
    if kw is None:
        s.field_stats_off()
    else:
        s.field_stats(1, **kw)


def measure(mg, n, nlevel, cycles, rounds):
    lat = mg.Lattice3d(n, n, n)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, 25.0), 5418513, mg.MultigridParameters(nlevel=nlevel))
    s.sample(16)
    times = {name: [] for name, _ in VARIANTS}
    paths = {}
    for _ in range(rounds):
        for name, kw in VARIANTS:
            enable(s, kw)
            paths[name] = s.field_cond_info()["path"]
            s.sample(8)
            times[name].append(s.sample_timed(cycles, stride=cycles)["total_ms"] / cycles)
    s.close()
    h = x_amplification(tile_constants())
    out = {"lattice": [n, n, n], "nlevel": nlevel, "cycles_per_round": cycles, "rounds": rounds, "paths": paths,
           "x_read_amplification": h, "variants": {}}
    for name, _ in VARIANTS:
        t = times[name]
        out["variants"][name] = {"cycle_ms_median": statistics.median(t), "cycle_ms_min": min(t), "cycle_ms_max": max(t),
                                 "cycle_ms_rounds": t}
    off = out["variants"]["off"]["cycle_ms_median"]
    for name, _ in VARIANTS[1:]:
        v = out["variants"][name]
        v["added_ms_per_cycle"] = v["cycle_ms_median"] - off
        v["added_fraction_of_cycle"] = v["added_ms_per_cycle"] / off
    plain = out["variants"]["plain"]["added_ms_per_cycle"]
    fused = out["variants"]["cond_fused"]["added_ms_per_cycle"]
    two = out["variants"]["cond_two_pass"]["added_ms_per_cycle"]
    out["fused_bytes_per_vertex"] = 8 * h + 32
    out["two_pass_bytes_per_vertex"] = 8 + 8 + 40
    out["fused_target_ms"] = plain * (8 * h + 32) / 40 * 1.15
    out["fused_meets_target"] = fused <= out["fused_target_ms"]
    out["fused_faster_than_two_pass"] = fused < two
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256:6,512:7")
    ap.add_argument("--cycles", type=int, default=0, help="cycles per timed window (0: by size)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_stats", "cond_cost.json"))
    ap.add_argument("--trace-run", default="", help="N:NLEVEL -- 32 cycles of each recording variant (for a kernel trace)")
    a = ap.parse_args()
    import multigridmc_amd as mg
    if a.trace_run:
        n, nlevel = (int(v) for v in a.trace_run.split(":"))
        s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(mg.Lattice3d(n, n, n), 25.0), 5418513,
                                  mg.MultigridParameters(nlevel=nlevel))
        for name, kw in VARIANTS[1:]:
            enable(s, kw)
            s.sample(32)
            print(f"{n}^3 {name}: {s.field_stats_info()['nrecorded']} states recorded, path {s.field_cond_info()['path']}")
        s.close()
        return
    results = []
    for item in a.sizes.split(","):
        n, nlevel = (int(v) for v in item.split(":"))
        cycles = a.cycles or (48 if n >= 512 else 200)
        r = measure(mg, n, nlevel, cycles, a.rounds)
        results.append(r)
        v = r["variants"]
        print(f"{n}^3 / {nlevel} levels: cycle off {v['off']['cycle_ms_median']:.4f} ms, plain "
              f"+{v['plain']['added_ms_per_cycle']:.4f}, conditional fused +{v['cond_fused']['added_ms_per_cycle']:.4f} "
              f"(target {r['fused_target_ms']:.4f}, h = {r['x_read_amplification']:.3f}), forced two-pass "
              f"+{v['cond_two_pass']['added_ms_per_cycle']:.4f} ms per cycle", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"library": os.environ.get("MGMC_LIBRARY", "product"), "results": results}, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
