#!/bin/bash
# The whole GPU suite under every launch-form knob of DESIGN.md section 6 (none of them may change a result).
#   tools/run_knob_matrix.sh [first [last]]   -- knobs first..last of the list (0-based), default all
# Stops at the first knob whose pytest run exits with anything but 0 or 1 (a time limit or a crash).
cd "$(dirname "$0")/.."
# Thirteen knobs are left: NZ_RCCL_LIB names a library; the other twelve FORCE a launch form at sizes where it is not
# the default, so that the small-grid parity tests cover every form that is the default somewhere.
KNOBS=(NZ_CONV_SYM=0 "NZ_CONV_SYM=0 NZ_CONV_SMALL=0" NZ_CONV_CHAIN=0 NZ_CONV_CHAIN=2 NZ_CONV_STREAM=0 NZ_CONV_STREAM=2 NZ_CONV_SMALL=0 NZ_CONV_SMALL=2 "NZ_CONV_SMALL=2 NZ_CONV_CHAIN=2"
       NZ_FLOW_STREAM=0 NZ_FLOW_STREAM=2 NZ_FLOW_FAIR=0 NZ_FLOW_FAIR=2 NZ_FLOW_TINY=0 NZ_FLOW_TINY=2 NZ_FLOW_TINY=3 NZ_FLOW_NMAX=1 NZ_FLOW_NMAX=3
       NZ_EROSION_EMAX=1 NZ_EROSION_EMAX=4 NZ_POOL_RUNS=0 NZ_POOL_SPARSE=0 NZ_POOL_SPARSE=2 NZ_PILE_TICKET=0)
first=${1:-0}; last=${2:-$((${#KNOBS[@]} - 1))}
for ((i = first; i <= last && i < ${#KNOBS[@]}; i++)); do
  kv=${KNOBS[$i]}
  echo "== $kv"
  log=gpurun_out/knob_$i.log
  mkdir -p gpurun_out
  env $kv timeout -k 10 600 python3 -m pytest tests -m gpu -q -rf > $log 2>&1
  rc=$?
  grep -E "^FAILED|^ERROR" $log
  tail -1 $log
  # 0: passed, 1: tests failed.  Anything else (124 / 137: time limit, 134: abort, 139: segfault, ...) may have left the
  # GPU faulted: start nothing more on it.
  if [ $rc -gt 1 ]; then
    echo "== $kv: pytest exited $rc -- stopping, no further knobs run"
    exit $rc
  fi
done
