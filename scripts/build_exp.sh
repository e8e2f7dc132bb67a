# Tuning builds of the library into build/ (never the product; select one with
# MGMC_LIBRARY=build/libmgmc_<name>.so).  The product sources carry no override switches: every
# launch-shape constant lives in multigridmc_amd/csrc/mgmc_tuning.hpp (tile shapes, chunk depths, thread
# counts, launch thresholds; tests/test_gpu_tuning.py checks that they change no bit).  A variant is a copy of
# the sources with some of those constants edited:
#   VARIANTS="ty16=ZS_TY:16 nt256=QUADS_NT:256,QUADS_NT3:256" bash scripts/build_exp.sh
# builds build/libmgmc_ty16.so and build/libmgmc_nt256.so.  CXXDEFS="-DMGMC_TAIL_PROF" adds
# compile definitions to every variant (the k_tail phase stamps of scripts/tail_prof.py).
# The recipe itself (copy, edit, the product's Makefile) is scripts/build_tuning_variants.py, shared with the
# test variants of tests/tuning_variants.py.
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
[ -n "${VARIANTS:-}" ] || exit 0
MGMC_EXP_CXXDEFS="${CXXDEFS:-}" python "$ROOT/scripts/build_tuning_variants.py" --exp $VARIANTS
