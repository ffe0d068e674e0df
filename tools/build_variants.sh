#!/bin/bash
# Build A/B variants of libbcmpc.so into build/variants/ (selected at run time via BCMPC_LIB).
# usage: tools/build_variants.sh [-p] "name:-DFLAG=1 ..." ...
#   default: flags apply to rollout.hip + rollout_grp.hip (f32 kernels)
#   -p     : flags apply to the three split-kernel units (rollout_x3_plain / rollout_x3 / rollout_pp, every
#            width and NC), each with its production scheduler
#   name@gitref (with -p): the split-kernel sources (rollout_x3.h, rollout_pp.h and the three units) at that
#            revision.  Revisions from before the sources were split into these files have another layout: build
#            a worktree of that revision (git worktree add DIR REF; make -C DIR) and pass its library as BCMPC_LIB.
# Every variant links the in-tree build's other objects and the host units rebuilt as a diagnostic build.
set -e
cd "$(dirname "$0")/.."
mkdir -p build/variants
H="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -DBCMPC_DIAG_VARIANT"
SPLIT="rollout_x3.h rollout_pp.h rollout_x3_plain.hip rollout_x3.hip rollout_pp.hip"
X3=0
if [ "${1:-}" = "-p" ]; then X3=2; shift; fi
make -s -j8 ARCH=gfx950 >/dev/null
HOST="capi engine_plan pack mt_draw planners"
HOSTOBJ=""
for u in $HOST; do
  $H -x hip -c bc_mpc_amd/csrc/$u.cpp -o build/variants/$u.o
  HOSTOBJ="$HOSTOBJ build/variants/$u.o"
done
# the in-tree build's objects except the host units and the named ones (the variant's own replace them)
others() { ls build/*.o | grep -v -E "/(${HOST// /|}|$1)\.o$"; }
link() { name=$1; shift; /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o build/variants/libbcmpc_$name.so "$@" $HOSTOBJ -ldl; }
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  src=bc_mpc_amd/csrc
  if [[ "$name" == *@* ]]; then     # name@gitref: the split-kernel sources at that revision, beside the tree's other headers
    ref=${name#*@}; name=${name%%@*}
    [ $X3 = 2 ] || { echo "$name@$ref: name@gitref needs -p" >&2; exit 2; }
    src=build/variants/src_$name
    mkdir -p $src
    for f in $SPLIT; do
      git show "$ref":bc_mpc_amd/csrc/$f > $src/$f 2>/dev/null || {
        echo "$ref has no bc_mpc_amd/csrc/$f: for a revision from before the split-kernel sources were split," \
             "build a worktree of it and pass its library as BCMPC_LIB" >&2; exit 2; }
    done
    flags="-I$PWD/bc_mpc_amd/csrc $flags"
  fi
  if [ $X3 = 2 ]; then
    ( $H -mllvm -amdgpu-sched-strategy=iterative-ilp $flags -c $src/rollout_x3_plain.hip -o build/variants/rollout_x3_plain_$name.o &&
      $H -mllvm -amdgpu-sched-strategy=max-ilp $flags -c $src/rollout_x3.hip -o build/variants/rollout_x3_$name.o &&
      $H -mllvm -amdgpu-sched-strategy=max-ilp $flags -c $src/rollout_pp.hip -o build/variants/rollout_pp_$name.o &&
      link $name $(others "rollout_x3|rollout_x3_plain|rollout_pp") build/variants/rollout_x3_$name.o \
           build/variants/rollout_x3_plain_$name.o build/variants/rollout_pp_$name.o ) &
  else
    ( $H $flags -c bc_mpc_amd/csrc/rollout.hip -o build/variants/rollout_$name.o &&
      $H $flags -c bc_mpc_amd/csrc/rollout_grp.hip -o build/variants/rollout_grp_$name.o &&
      link $name $(others "rollout|rollout_grp") build/variants/rollout_$name.o build/variants/rollout_grp_$name.o ) &
  fi
done
wait
rm -rf build/variants/src_*
ls build/variants/*.so
