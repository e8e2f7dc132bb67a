"""Re-tuned builds of the library for the tuning-neutrality tests: variant name -> {constant: value}.

Each variant is the product sources with these `constexpr int` values of multigridmc_amd/csrc/mgmc_tuning.hpp
replaced (scripts/build_tuning_variants.py builds build/libmgmc_tune_<name>.so with the product's flags).
tests/test_tuning_host.py checks on the CPU that every constant of the header is non-default in at least one
variant and that the variants select the kernel instances the cases are there for; tests/test_gpu_tuning.py runs
the parity cases through each library on the GPU.  Values stay inside the domains the sources assert
(ZS_TY % 4 == 0 and <= 32, ZS_TZ / ZS_TZP even at every halving down to 8, JS_D in 2 .. 4, ...)."""

VARIANTS = {
    "lo": {
        "ZS_TY": 16, "ZS_MINW": 4, "ZS_TZ": 16, "ZS_TYP": 12, "ZS_MINWP": 5, "ZS_TZP": 32,
        "QUADS_MAXPAIR": 32, "QUADS_LANES": 0, "QUADS_NT": 256, "QUADS_NT3": 256,
        # (JS_ROUNDS changes a launch only where a half's planes x steps exceed one round of resident workgroups:
        # the case 3d_jsweep_rounds of tests/test_gpu_tuning.py)
        "JS_D": 2, "JS_ROUNDS": 2,
        "ZR7_WIDE_MIN_TILES": 1, "ZR_SMALL_NX": 16, "ZR27_CY": 8, "ZR27_MINW": 2,
        "PROLONG_Z": 4, "PROLONG_Z_SMALL": 2, "TAIL_PN_WG": 0,
        # (LR_STAGED_MAX_WAVES 1: every dot product runs k_lr_partials, so its entries-per-lane and
        # chains-per-wavefront constants are varied here)
        "LR_STAGED_MAX_WAVES": 1, "LR_PART_U": 4, "LR_PART_CH": 2, "LR_DENSE_PER": 4,
        "FS_NT": 128, "FS_PAIRS": 2,
    },
    "hi": {
        "ZS_TY": 28, "ZS_TZ": 64, "ZS_TYP": 20, "ZS_TZP": 64,
        "QUADS_MAXPAIR": 128, "QUADS_NT_WIDE": 512, "JS_D": 4,
        "ZR_SMALL_NX": 64, "ZR7_WIDE_MIN_TILES": 1073741824, "ZR27_CX": 32,
        "PROLONG_Z": 16, "TAIL_PN_WG": 255,
        # (LR_STAGED_MAX_WAVES 2^20: every dot product runs the staged kernel, which is what this variant tests of
        # the low-rank dots; LR_PART_U and LR_PART_CH belong to k_lr_partials and are inert here -- "lo" varies them)
        "LR_STAGED_MAX_WAVES": 1048576, "LR_PART_U": 16, "LR_PART_CH": 2, "LR_DENSE_PER": 16,
        "FS_NT": 512,
    },
}
