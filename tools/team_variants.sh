#!/bin/bash
# Build A/B or diagnostic variants of the team kernel (rollout_team.hip) into
# build/variants/libbcmpc_<name>.so (selected at run time via BCMPC_LIB).
# usage: tools/team_variants.sh "name:-DFLAG=1 ..." ...
set -e
cd "$(dirname "$0")/.."
mkdir -p build/variants
H="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -DBCMPC_DIAG_VARIANT"
make -s -j8 ARCH=gfx950 >/dev/null
HOST="capi engine_plan pack mt_draw planners"
# the in-tree build's other objects
OBJS=$(ls build/*.o | grep -v -E "/(${HOST// /|}|rollout_team)\.o$")
# the host units are rebuilt with each variant's flags: the host weight packing (pack.cpp) and the kernel must agree
# on the compile-time switches they share (TEAM_DEFER: the output layer packed for the deferred LayerNorm or not)
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  ( $H ${TEAMSCHED:--mllvm -amdgpu-sched-strategy=iterative-ilp} $flags -c bc_mpc_amd/csrc/rollout_team.hip -o build/variants/rollout_team_$name.o &&
    for u in $HOST; do $H $flags -x hip -c bc_mpc_amd/csrc/$u.cpp -o build/variants/${u}_team_$name.o || exit 1; done &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o build/variants/libbcmpc_$name.so $OBJS \
        $(for u in $HOST; do echo build/variants/${u}_team_$name.o; done) build/variants/rollout_team_$name.o -ldl ) &
done
wait
ls build/variants/*.so
