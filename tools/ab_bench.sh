#!/bin/bash
# A/B of library builds on the bench workload in one session, sides alternating (a, b, a, b, ...): one line per run, in the
# form kept under profiles/ (median_hipevent = config.ms_per_step_median_hipevent_rank0; plan / fwd / bwd / ties = stage_ms_rank0).
#   tools/ab_bench.sh ROUNDS "parent=dmesh2_renderer_amd/csrc/ab/lib_parent.so new=dmesh2_renderer_amd/csrc/libdm2_hip.so" [bench.py arguments ...]
# Stops at the first run that fails.
ROUNDS=$1; SIDES=$2; shift 2
CMD="bench.py --no-cpu --steps 20 --warmup 5 $*"
for i in $(seq "$ROUNDS"); do for side in $SIDES; do
  out=$(DM2_HIP_LIB=$PWD/${side#*=} timeout -k 10 300 python $CMD 2>/dev/null | tail -1) || { echo "$CMD | ${side%%=*} | failed"; exit 1; }
  echo "$out" | python -c "
import sys, json
d = json.loads(sys.stdin.read()); c = d['config']; s = c['stage_ms_rank0']
print('$CMD | ${side%%=*} | median_hipevent', c['ms_per_step_median_hipevent_rank0'], 'ms_per_step', d['ms_per_step'], 'plan', s['preprocess_scan'], 'fwd', s['forward_composite'], 'bwd', s['backward_composite'], 'ties', s.get('backward_ties'))" || exit 1
done; done
