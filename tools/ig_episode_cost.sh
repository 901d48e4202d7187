#!/bin/bash
# Kernel times of the cfg5 step with the IG episode boundary (tools/ig_episode_cost.py): --reps rocprofv3 --kernel-trace runs of
# the episodic env under auto-reset, each under its own time limit, every run summarised on its own (the spread between the
# runs' planner times is the session's run-to-run spread).  A second argument names the root of another checkout of the project,
# built (e.g. the parent commit's): its default attach is stepped the same way for the planner's A/B.
set -o pipefail
# usage: tools/ig_episode_cost.sh [out_dir] [other_checkout_root]
O=${1:-exp_out/ig_episode_cost}
ALT=$2
STEPS=6
FORCED=4
HERE=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$O"
O=$(cd "$O" && pwd)
for rep in 1 2; do
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/this_$rep" -o run -- \
    python3 "$HERE/tools/ig_episode_cost.py" --steps $STEPS --forced $FORCED > "$O/this_$rep.jsonl" &&
  cat "$O/this_$rep.jsonl" &&
  python3 "$HERE/tools/ig_episode_cost.py" --summarize "$O/this_$rep" --steps $STEPS --forced $FORCED | tee "$O/this_$rep.summary.json" || exit 1
  if [ -n "$ALT" ]; then
    timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/alt_$rep" -o run -- \
      python3 "$HERE/tools/ig_episode_cost.py" --steps $STEPS --episodic 0 --root "$ALT" > "$O/alt_$rep.jsonl" &&
    cat "$O/alt_$rep.jsonl" &&
    python3 "$HERE/tools/ig_episode_cost.py" --summarize "$O/alt_$rep" --steps $STEPS --forced 0 | tee "$O/alt_$rep.summary.json" || exit 1
  fi
done
