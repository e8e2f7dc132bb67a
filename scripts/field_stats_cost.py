"""What the pointwise field statistics (MultigridMCSampler.field_stats, mgmc_fieldstats.hpp) add to a cycle.

For each lattice (default 3D 256^3 / 6 levels and 512^3 / 7 levels, the prior with f = 0: bench.py's
workload) one sampler runs three variants in one process, interleaved round by round: statistics off,
stride 1 and stride 8.  A round of a variant is `cycles` cycles (a multiple of 8, so a stride-8 window holds
cycles / 8 recorded cycles) timed with sample_timed -- HIP events on the handle's stream, total = first to
last event -- after 8 untimed cycles of the variant.  Reported per variant: the median and the spread of the
cycle time over the rounds; for stride 1 also the added time per cycle against "off", the bytes the kernel
moves per recorded cycle, (8 K + 32) x nstore for K chains, and the bytes per second and the fraction of
the measured stream ceiling (profiles/r01_stream_ceiling.txt: 6.0 TB/s) that this added time amounts to.  The
added time holds the kernel, its one-thread counter launch and their two launch boundaries.

    python scripts/field_stats_cost.py [--sizes 256:6,512:7] [--cycles N] [--rounds R] [--nchains K]
                                       [--out profiles/field_stats/cost.json]

The kernel's own time comes from a kernel trace, taken in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/field_stats_cost.py --trace-run 512:7
runs 32 cycles with stride 1 and nothing else; scripts/kstats.py DIR/.../kt_kernel_trace.csv 32 lists k_fieldstats.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_CEILING = 6.0e12  # bytes / s, profiles/r01_stream_ceiling.txt (triad, full grid)
VARIANTS = (("off", 0), ("stride1", 1), ("stride8", 8))


def nstore_3d(n):
    """doubles of the fine level's padded layout (make_layout, mgmc_kernels.hpp)"""
    sx = (n + 16 + 15) // 16 * 16
    return sx * (n + 1) * (n + 1) + 64


def measure(mg, n, nlevel, cycles, rounds, nchains):
    lat = mg.Lattice3d(n, n, n)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, 25.0), 5418513, mg.MultigridParameters(nlevel=nlevel),
                              nchains=nchains)
    s.sample(16)
    times = {name: [] for name, _ in VARIANTS}
    for _ in range(rounds):
        for name, stride in VARIANTS:
            if stride:
                s.field_stats(stride)  # (on an enabled handle: a reset with the new stride)
            else:
                s.field_stats_off()
            s.sample(8)
            # (stride = cycles: only the first and the last cycle carry event records; the total runs from
            # before the first cycle's first kernel to after the last cycle's last)
            times[name].append(s.sample_timed(cycles, stride=cycles)["total_ms"] / cycles)
    recorded = s.field_stats_info()
    s.close()
    ns = nstore_3d(n)
    out = {"lattice": [n, n, n], "nlevel": nlevel, "nchains": nchains, "nstore": ns, "cycles_per_round": cycles,
           "rounds": rounds, "last_window": recorded, "variants": {}}
    for name, _ in VARIANTS:
        t = times[name]
        out["variants"][name] = {"cycle_ms_median": statistics.median(t), "cycle_ms_min": min(t), "cycle_ms_max": max(t),
                                 "cycle_ms_rounds": t}
    off = out["variants"]["off"]["cycle_ms_median"]
    bytes_per_record = (8 * nchains + 32) * ns
    for name, stride in VARIANTS[1:]:
        v = out["variants"][name]
        v["added_ms_per_cycle"] = v["cycle_ms_median"] - off
        v["added_ms_per_recorded_cycle"] = v["added_ms_per_cycle"] * stride
        v["added_fraction_of_cycle"] = v["added_ms_per_cycle"] / off
    v = out["variants"]["stride1"]
    out["bytes_per_recorded_cycle"] = bytes_per_record
    if v["added_ms_per_cycle"] > 0:
        rate = bytes_per_record / (v["added_ms_per_cycle"] * 1e-3)
        out["stride1_bytes_per_s"] = rate
        out["stride1_fraction_of_stream_ceiling"] = rate / STREAM_CEILING
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256:6,512:7")
    ap.add_argument("--cycles", type=int, default=0, help="cycles per timed window (multiple of 8; 0: by size)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--nchains", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_stats", "cost.json"))
    ap.add_argument("--trace-run", default="", help="N:NLEVEL -- 32 cycles with stride 1 only (for a kernel trace)")
    a = ap.parse_args()
    import multigridmc_amd as mg
    if a.trace_run:
        n, nlevel = (int(v) for v in a.trace_run.split(":"))
        s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(mg.Lattice3d(n, n, n), 25.0), 5418513,
                                  mg.MultigridParameters(nlevel=nlevel), nchains=a.nchains)
        s.field_stats(1)
        s.sample(32)
        print(f"{n}^3: {s.field_stats_info()['nrecorded']} states recorded; "
              f"{(8 * a.nchains + 32) * nstore_3d(n)} bytes per recorded cycle")
        s.close()
        return
    results = []
    for item in a.sizes.split(","):
        n, nlevel = (int(v) for v in item.split(":"))
        cycles = a.cycles or (48 if n >= 512 else 200)
        if cycles % 8:
            ap.error("--cycles must be a multiple of 8")
        r = measure(mg, n, nlevel, cycles, a.rounds, a.nchains)
        results.append(r)
        v = r["variants"]
        print(f"{n}^3 / {nlevel} levels, {a.nchains} chain(s): cycle off {v['off']['cycle_ms_median']:.4f} ms, "
              f"stride 1 {v['stride1']['cycle_ms_median']:.4f} ms (+{v['stride1']['added_ms_per_cycle']:.4f}), "
              f"stride 8 {v['stride8']['cycle_ms_median']:.4f} ms (+{v['stride8']['added_ms_per_cycle']:.4f}); "
              f"stride 1: {r.get('stride1_bytes_per_s', 0.0) / 1e12:.2f} TB/s = "
              f"{100 * r.get('stride1_fraction_of_stream_ceiling', 0.0):.0f}% of the stream ceiling", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"library": os.environ.get("MGMC_LIBRARY", "product"), "stream_ceiling_bytes_per_s": STREAM_CEILING,
                   "results": results}, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
