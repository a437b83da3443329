#!/bin/bash
# Same-box A/B of environment settings on the default bench: tools/ab_env.sh REPS OUT "A=1" "A=0" ...  (alternating runs, one line each)
# Each line: pairs/s, ms/step, and what the last timed step computed (it starts from the seeded state in every run, see bench.py StartState):
# its loss, the L2 norm of its gradients and the sum of the weights after its Adam update (--dump-outputs) -- equal settings give equal
# numbers up to rounding, so a variant that changes backward or the optimiser shows there.
REPS=$1; OUT=$2; shift; shift
for i in $(seq $REPS); do
  for cfg in "$@"; do
    dump=$(mktemp -d)
    env $cfg python bench.py --steps 40 --warmup 5 --dump-outputs $dump 2>&1 | tail -1 | python -c "import sys,json,numpy as np; d=json.loads(sys.stdin.read()); g=np.load('$dump/gradients.npy').astype(np.float64); p=np.load('$dump/parameters.npy').astype(np.float64); print('$cfg', round(d['value'],1), round(d['ms_per_step'],3), d['config']['final_loss'], 'grad_l2', float(np.linalg.norm(g)), 'param_sum', float(p.sum()), flush=True)" >> $OUT
    rm -rf $dump
  done
done
cat $OUT
