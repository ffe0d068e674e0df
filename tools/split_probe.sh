#!/bin/bash
# Register / spill / LDS report for single instantiations of the split kernels (no launchers, seconds per build).
# usage: tools/split_probe.sh KERNEL ... [-- extra hipcc flags, e.g. -DPP_D=3 -DPP3_PRIO_M=0]
#   KERNEL: x3:HP,NC,NW,PHP,RW,AK,F1   rollout_x3<...>            (rollout_x3.h)
#           pp[:FOLD]                  rollout_pp<512, FOLD=true>  (rollout_pp.h)
#           pp3                        rollout_pp3<512>            (rollout_pp.h)
# Scheduler: max-ILP unless $X3SCHED names another (the plain unit's: "-mllvm -amdgpu-sched-strategy=iterative-ilp").
set -e -o pipefail
cd "$(dirname "$0")/.."
insts=(); extra=()
while [ $# -gt 0 ]; do
  if [ "$1" = "--" ]; then shift; extra=("$@"); break; fi
  insts+=("$1"); shift
done
[ ${#insts[@]} -gt 0 ] || { sed -n '2,7p' "$0"; exit 2; }
f=$(mktemp /tmp/splitprobe_XXXX.hip)
{
  echo '#include "'$PWD'/bc_mpc_amd/csrc/rollout_pp.h"'
  for i in "${insts[@]}"; do
    case $i in
      x3:*) echo "template __global__ void bcmpc::rollout_x3<${i#x3:}>(const bcmpc::RolloutArgs);" ;;
      pp)   echo "template __global__ void bcmpc::rollout_pp<512, true>(const bcmpc::RolloutArgs);" ;;
      pp:*) echo "template __global__ void bcmpc::rollout_pp<512, ${i#pp:}>(const bcmpc::RolloutArgs);" ;;
      pp3)  echo "template __global__ void bcmpc::rollout_pp3<512>(const bcmpc::RolloutArgs);" ;;
      *)    echo "unknown kernel $i" >&2; exit 2 ;;
    esac
  done
} > $f
log=${f%.hip}.log
trap 'rm -f $f ${f%.hip}.o $log' EXIT
# (a compile error, e.g. a mistyped template argument, is shown and fails the script: the report's filter would hide it)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize \
  ${X3SCHED:--mllvm -amdgpu-sched-strategy=max-ilp} "${extra[@]}" --cuda-device-only -c $f -o ${f%.hip}.o \
  -Rpass-analysis=kernel-resource-usage > $log 2>&1 || { grep -v "remark:" $log >&2; exit 1; }
grep -E "Function Name|VGPRs:|AGPRs:|Spill|ScratchSize|Occupancy|LDS Size" $log | \
  sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//' | paste - - - - - - - - | sed 's/Function Name: _ZN5bcmpc1[01]//'
