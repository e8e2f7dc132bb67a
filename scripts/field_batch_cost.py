"""What the batch means of the field statistics (MultigridMCSampler.field_stats(stride, batch=B), the instance
k_fieldstats<NCH, true> of mgmc_fieldstats.hpp) add to a cycle, next to the statistics without them and to the parent
commit's library.

For each lattice (default 3D 256^3 / 6 levels and 512^3 / 7 levels, the prior with f = 0: bench.py's workload) one
process holds two samplers on the head's library and, where --parent names one, two on the parent's
(build/libmgmc_parent.so: the parent commit's multigridmc_amd/csrc and include compiled with the product's flags,
DESIGN.md section 8 "Parent against head"), and runs these variants interleaved, round by round:

    parent_off, parent_stride1                     the parent's library: statistics off / stride 1
    parent2_off, parent2_stride1                   the same library on a second sampler of its own: what two handles
                                                   of one library differ by (their buffers lie elsewhere in HBM)
    off, stride1                                   the head's library: the same, on a sampler that goes through the
                                                   allocations the parent's samplers go through and no others
    batch_off, batch16_stride1, batch16_stride8    the head's library, its second sampler: statistics off / batch
                                                   means of 16 recorded cycles

A round of a variant is `cycles` cycles (a multiple of 128 = 8 x 16, so a stride-8 window holds whole batches) timed
with sample_timed -- HIP events on the handle's stream, total = first to last event -- after 16 untimed cycles of
the variant.  Per variant: the median, the extremes and the spread (max - min) / median of the cycle time over the
rounds.  For the statistics variants the time added against "off" of the same sampler; for batch16_stride1 the bytes
of the mid-batch path, (8 K + 48) x nstore per recorded cycle, and of the window's average (one cycle in 16 ends a
batch: 8 K + 80), over that added time.  The added time holds the kernel, its one-thread counter launch and their
launch boundaries; inside the replayed graph it is not the kernel's own time.

The condition on the parent's behaviour: the head's "off" and "stride1" medians differ from the parent's medians by
no more than the parent's own spread over the rounds (its slowest round minus its fastest), recorded under
agrees_with_parent together with whether the head's median lies between the parent's extremes; a failure is
reported as such and the exit status is 2.

    python scripts/field_batch_cost.py [--sizes 256:6,512:7] [--cycles N] [--rounds R] [--nchains K]
                                       [--parent build/libmgmc_parent.so | --parent ""]
                                       [--out profiles/field_stats/batch_cost.json]

The kernels' own times come from a kernel trace, taken in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/field_batch_cost.py --trace-run 512:7
runs 32 cycles with stride 1 and then 32 cycles with stride 1 and batches of 16 on the head's library and nothing
else: 32 launches of k_fieldstats<1, false>, then 32 of k_fieldstats<1, true>, of which the 16th and the 32nd end a batch.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 5418513
STREAM_CEILING = 6.0e12  # bytes / s, profiles/r01_stream_ceiling.txt (triad, full grid)
BATCH = 16
# name -> (library, stride (0: off), batch (None: without batching))
VARIANTS = (("parent_off", "parent", 0, None), ("parent_stride1", "parent", 1, None),
            ("parent2_off", "parent2", 0, None), ("parent2_stride1", "parent2", 1, None), ("off", "head", 0, None),
            ("stride1", "head", 1, None), ("batch_off", "head2", 0, None), ("batch16_stride1", "head2", 1, BATCH),
            ("batch16_stride8", "head2", 8, BATCH))
OFF = {"parent": "parent_off", "parent2": "parent2_off", "head": "off", "head2": "batch_off"}


def nstore_3d(n):
    """doubles of the fine level's padded layout (make_layout, mgmc_kernels.hpp)"""
    sx = (n + 16 + 15) // 16 * 16
    return sx * (n + 1) * (n + 1) + 64


def load(path):
    """libmgmc of `path` with every symbol it has bound (the parent's library lacks the newer entries)."""
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


def measure(mg, libs, n, nlevel, cycles, rounds, nchains):
    from multigridmc_amd import _native
    samplers = {}
    for name, lib in libs.items():
        _native._lib = lib  # (the package binds its samplers to the library loaded at their creation)
        samplers[name] = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(mg.Lattice3d(n, n, n), 25.0), SEED,
                                               mg.MultigridParameters(nlevel=nlevel), nchains=nchains)
        samplers[name].sample(16)
    variants = [v for v in VARIANTS if v[1] in samplers]
    times = {v[0]: [] for v in variants}
    for r in range(rounds):
        for name, which, stride, batch in variants:
            s = samplers[which]
            if not stride:
                s.field_stats_off()
            elif batch is None:
                s.field_stats(stride)
            else:
                s.field_stats(stride, batch=batch)
            s.sample(16)
            # (stride = cycles: only the first and the last cycle carry event records)
            times[name].append(s.sample_timed(cycles, stride=cycles)["total_ms"] / cycles)
        print(f"  round {r}: " + ", ".join(f"{name} {times[name][-1]:.4f}" for name, _, _, _ in variants), flush=True)
    last = samplers["head2"].field_batch_info()
    for s in samplers.values():
        s.close()
    ns = nstore_3d(n)
    out = {"lattice": [n, n, n], "nlevel": nlevel, "nchains": nchains, "nstore": ns, "cycles_per_round": cycles,
           "rounds": rounds, "batch": BATCH, "last_window": last, "variants": {}}
    for name, which, stride, batch in variants:
        t = times[name]
        med = statistics.median(t)
        out["variants"][name] = {"library": which, "stride": stride, "batch": batch or 0, "cycle_ms_median": med,
                                 "cycle_ms_min": min(t), "cycle_ms_max": max(t), "spread": (max(t) - min(t)) / med,
                                 "cycle_ms_rounds": t}
    v = out["variants"]
    for name, which, stride, batch in variants:
        if stride:
            off = v[OFF[which]]["cycle_ms_median"]
            v[name]["added_ms_per_cycle"] = v[name]["cycle_ms_median"] - off
            v[name]["added_ms_per_recorded_cycle"] = v[name]["added_ms_per_cycle"] * stride
            v[name]["added_fraction_of_cycle"] = v[name]["added_ms_per_cycle"] / off
    for name, per_vertex in (("stride1", 8 * nchains + 32), ("batch16_stride1", 8 * nchains + 48)):
        e = v[name]
        e["bytes_per_recorded_cycle"] = per_vertex * ns
        if e["added_ms_per_cycle"] > 0:
            e["bytes_per_s"] = e["bytes_per_recorded_cycle"] / (e["added_ms_per_cycle"] * 1e-3)
            e["fraction_of_stream_ceiling"] = e["bytes_per_s"] / STREAM_CEILING
    e = v["batch16_stride1"]
    e["bytes_per_cycle_window_average"] = (8 * nchains + 48 + 32.0 / BATCH) * ns
    if e["added_ms_per_cycle"] > 0:
        e["bytes_per_s_window_average"] = e["bytes_per_cycle_window_average"] / (e["added_ms_per_cycle"] * 1e-3)
    if "parent" in samplers:
        agree = {}
        for mine, theirs in (("off", "parent_off"), ("stride1", "parent_stride1")):
            p = v[theirs]
            agree[mine] = {"head_median": v[mine]["cycle_ms_median"], "parent_min": p["cycle_ms_min"],
                           "parent2_median": v[theirs.replace("parent", "parent2")]["cycle_ms_median"],
                           "parent_max": p["cycle_ms_max"], "parent_median": p["cycle_ms_median"],
                           "head_over_parent": v[mine]["cycle_ms_median"] / p["cycle_ms_median"],
                           "between_parent_extremes": p["cycle_ms_min"] <= v[mine]["cycle_ms_median"] <= p["cycle_ms_max"],
                           "within_parent_spread": abs(v[mine]["cycle_ms_median"] - p["cycle_ms_median"])
                           <= p["cycle_ms_max"] - p["cycle_ms_min"]}
        out["agrees_with_parent"] = agree
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256:6,512:7")
    ap.add_argument("--cycles", type=int, default=0, help="cycles per timed window (multiple of 128; 0: by size)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--nchains", type=int, default=1)
    ap.add_argument("--parent", default=os.path.join(ROOT, "build", "libmgmc_parent.so"),
                    help="the parent commit's library; empty: the head's variants only")
    ap.add_argument("--head", default=os.path.join(ROOT, "multigridmc_amd", "libmgmc_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_stats", "batch_cost.json"))
    ap.add_argument("--trace-run", default="", help="N:NLEVEL -- 32 + 32 cycles on --head only (for a kernel trace)")
    a = ap.parse_args()
    if a.trace_run:
        import multigridmc_amd as mg
        from multigridmc_amd import _native
        n, nlevel = (int(v) for v in a.trace_run.split(":"))
        _native._lib = load(a.head)
        s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(mg.Lattice3d(n, n, n), 25.0), SEED,
                                  mg.MultigridParameters(nlevel=nlevel), nchains=a.nchains)
        s.field_stats(1)
        s.sample(32)
        s.field_stats(1, batch=BATCH)
        s.sample(32)
        print(f"{n}^3: {s.field_batch_info()}; nstore {nstore_3d(n)}: {(8 * a.nchains + 32) * nstore_3d(n)} bytes per "
              f"recorded cycle without batching, {(8 * a.nchains + 48) * nstore_3d(n)} mid-batch, "
              f"{(8 * a.nchains + 80) * nstore_3d(n)} at a batch end")
        s.close()
        return
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import multigridmc_amd as mg
    libs = {}
    libs["head"] = libs["head2"] = load(a.head)
    if a.parent:
        libs["parent"] = libs["parent2"] = load(a.parent)
    results, ok = [], True
    for item in a.sizes.split(","):
        n, nlevel = (int(v) for v in item.split(":"))
        cycles = a.cycles or (128 if n >= 512 else 256)
        if cycles % (8 * BATCH):
            ap.error("--cycles must be a multiple of 128")
        print(f"{n}^3 / {nlevel} levels, {a.nchains} chain(s), {cycles} cycles per window:", flush=True)
        r = measure(mg, libs, n, nlevel, cycles, a.rounds, a.nchains)
        results.append(r)
        v = r["variants"]
        print(f"  off {v['off']['cycle_ms_median']:.4f} ms; stride 1 +{v['stride1']['added_ms_per_cycle']:.4f}; "
              f"batch 16, stride 1 +{v['batch16_stride1']['added_ms_per_cycle']:.4f} "
              f"({v['batch16_stride1'].get('bytes_per_s', 0.0) / 1e12:.2f} TB/s on the mid-batch bytes); "
              f"batch 16, stride 8 +{v['batch16_stride8']['added_ms_per_cycle']:.4f}", flush=True)
        for name, g in r.get("agrees_with_parent", {}).items():
            ok = ok and g["within_parent_spread"]
            print(f"  {name}: head {g['head_median']:.4f} ms, parent {g['parent_median']:.4f} ms "
                  f"({g['parent_min']:.4f} .. {g['parent_max']:.4f}; its second sampler {g['parent2_median']:.4f}): "
                  f"{'within' if g['within_parent_spread'] else 'OUTSIDE'} the parent's spread", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"parent_library": os.path.relpath(a.parent, ROOT) if a.parent else None,
                   "stream_ceiling_bytes_per_s": STREAM_CEILING, "head_agrees_with_parent": ok if a.parent else None,
                   "results": results}, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")
    if not ok:
        sys.exit(2)


if __name__ == "__main__":
    main()
