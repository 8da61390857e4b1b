#!/bin/bash
# Builds halo2-plonky2-verifier_amd/libh2w_<name>.so: the same sources with the extra compiler flags in H2W_EXTRA (compile-time knobs of the
# kernels: -DH2W_FAST_T=8, -DH2W_QUAD_BLOCK=512, ...; or whatever a local experiment patch reads).  Usage: H2W_EXTRA="..." build_debug_variant.sh [name=dbg].
# H2W_UNITS: the units compiled with the flags (default: the three kernel units the knobs are read in; the lowering dump, -DH2W_LOWERING_DUMP, is read
# in "traceplan.cpp" alone, and a comparison of two lowerings wants "traceplan.cpp tracelower.cpp"); every other object is the product build's (build.sh first).
# Select it with H2W_LIB=<path> (tools/experiments/variant.sh does both).  Never used by tests, smoke or the default bench.
set -e
name=${1:-dbg}
cd "$(dirname "$0")/../halo2-plonky2-verifier_amd/csrc"
FLAGS="$H2W_EXTRA -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -Wno-unused-value -x hip"
units=${H2W_UNITS:-batch.hip glue.hip expand.hip}
mkdir -p ../build_$name
for f in $units; do hipcc $FLAGS -c $f -o ../build_$name/${f%.*}.o; done
objs=""
for u in expand eager plancompile batch advicetools glue chipbatch chiphash chipvalues abi_backend prover comm replay traceplan bnemit_mont tracelower verdict traceverdict merkletree; do
  case " $units " in *" $u.hip "*|*" $u.cpp "*) objs="$objs ../build_$name/$u.o";; *) objs="$objs ../build/$u.o";; esac
done
hipcc --offload-arch=gfx950 -shared -fPIC $objs -ldl -o ../libh2w_$name.so
echo "built $(realpath ../libh2w_$name.so)"
