#!/bin/bash
# tuning aid: builds engine variants skirt9_amd/lib/libpmc_<name>.so (make variant) in parallel
#   tools/build_variants.sh "refill32 -DPMC_PROP_REFILL=32" "steps4 -DPMC_WALK_STEPS=4" ...
# (the perturbation, ablation and fold-octant variants need their patch from profiles/experiments applied first:
#  git apply profiles/experiments/perturb_octree_step.patch, ablate_walk_side, ablate_transition_side, fold_octant)
cd "$(dirname "$0")/.."
n=0
for v in "$@"; do
  set -- $v; name=$1; shift
  make -s variant NAME=$name DEFS="$*" 2>&1 | grep -v "warning\|^ *[0-9]* |\|\^\|generated" &
  n=$((n+1)); if [ $((n % 6)) = 0 ]; then wait; fi
done
wait
ls -la skirt9_amd/lib/ | awk '{print $5, $9}'
