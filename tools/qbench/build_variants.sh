#!/bin/bash
# tools/qbench/build_variants.sh name=DEFS ... — one qbench binary per variant of the design-Q kernel (csrc/sdrfm_q.hip compiled with the given -D flags), e.g.
#   bash tools/qbench/build_variants.sh prod= base="-DSDRFM_Q_K3=0 -DSDRFM_Q_XORSKIP=0" m2=-DSDRFM_Q_MAGIC=2
# The arms of profiles/q_scalefree_experiments.txt (the scale-free recombination, the sixth window piece, the step's constants in VGPRs at four and at three waves per SIMD):
#   bash tools/qbench/build_variants.sh off="-DSDRFM_Q_SCALEFREE=0 -DSDRFM_Q_NOB6=0" sf=-DSDRFM_Q_NOB6=0 sfb= a15=-DSDRFM_Q_CVGPR=15 \
#        b15="-DSDRFM_Q_CVGPR=15 -DSDRFM_Q_W3=1" b31="-DSDRFM_Q_CVGPR=31 -DSDRFM_Q_W3=1"
# (a parent commit's binary: build tools/qbench in a checkout of that commit and copy its qbench here as qbench_parent)
# The binaries (qbench_<name>, git-ignored) travel to the GPU box with the snapshot; tools/ab.sh runs them in turn on one box.
cd "$(dirname "$0")" || exit 1
for spec in "$@"; do
  name=${spec%%=*}; defs=${spec#*=}
  make -s clean >/dev/null; make -s QDEFS="$defs" qbench 2>&1 | grep -vE 'warning: argument unused|^$' ; mv qbench qbench_$name && echo "built qbench_$name [$defs]"
done
