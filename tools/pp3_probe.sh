#!/bin/bash
# Register / spill report for rollout_pp3<512> under extra flags (e.g. -DPP3_PRIO_M=0).
# usage: tools/pp3_probe.sh [hipcc flags...]
set -e
cd "$(dirname "$0")/.."
f=$(mktemp /tmp/pp3probe_XXXX.hip)
{ echo '#define X3_PROBE 1'; echo '#include "'$PWD'/bc_mpc_amd/csrc/rollout_x3.hip"'
  echo "template __global__ void bcmpc::rollout_pp3<512>(const bcmpc::RolloutArgs);"; } > $f
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize \
  ${X3SCHED:--mllvm -amdgpu-sched-strategy=max-ilp} "$@" --cuda-device-only -c $f -o /tmp/pp3probe.o \
  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|AGPRs:|Spill|ScratchSize|Occupancy|LDS Size" | \
  sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - - - - | sed 's/Function Name: _ZN5bcmpc11//'
rm -f $f
