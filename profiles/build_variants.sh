#!/bin/bash
# kernel-tuning helper: build/variants/lib_<tag>.so = the library with multicorrelator.hip and multicorrelator_t128.hip (the kernel text of csrc/mcorr_kernels.h at 256 and at 128 threads: the headline
# kernel of bench.py) recompiled under extra -D flags
# usage: bash profiles/build_variants.sh t64:-DGSH_MC_THREADS=64 queue1:-DGSH_MC_PAIR_QUEUE=1 nobarrier:-DGSH_MC_PAIR_QUEUE=2,-DGSH_MC_PAIR_BARRIER=0 ...
set -e
R=$(cd $(dirname $0)/.. && pwd); P=$R/gnss-sdr_amd
python -c "import sys; sys.path.insert(0,'$R'); import gnss_sdr_amd; gnss_sdr_amd.build_library()"
mkdir -p $R/build/variants
for spec in "$@"; do
  tag=${spec%%:*}; defs=${spec#*:}; defs=${defs//,/ }
  for unit in multicorrelator multicorrelator_t128; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-function -I$R/include -I$P/csrc $defs -c $P/csrc/$unit.hip -o $R/build/variants/${unit}_$tag.o 2>/dev/null &
  done
  wait
  objs=$(ls $P/_build/*.o | grep -v "/multicorrelator.o\|/multicorrelator_t128.o")
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/build/variants/lib_$tag.so $objs $R/build/variants/multicorrelator_$tag.o $R/build/variants/multicorrelator_t128_$tag.o
  echo built lib_$tag.so "($defs)"
done
