#!/bin/bash
# Kernel times of the Dec-MCTS planning step in both modes at 2048 and 256 worlds (tools/dmcts_modes.py), one rocprofv3
# --kernel-trace --stats run per world count, each under its own time limit.  A second argument names another library build
# (e.g. the parent commit's) whose sequential kernel is timed the same way for an A/B.
# usage: tools/dmcts_modes.sh [out_dir] [other_libcagym_hip.so]
O=${1:-exp_out/dmcts_modes}
ALT=$2
mkdir -p "$O"
for n in 2048 256; do
  timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/w$n" -o run -- \
    python3 tools/dmcts_modes.py --worlds $n --reps 5 > "$O/w$n.jsonl" || exit 1
  cat "$O/w$n.jsonl"
  if [ -n "$ALT" ]; then
    CAGYM_LIB="$ALT" timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/alt_w$n" -o run -- \
      python3 tools/dmcts_modes.py --worlds $n --reps 5 --modes seq > "$O/alt_w$n.jsonl" || exit 1
    cat "$O/alt_w$n.jsonl"
  fi
done
for f in $(find "$O" -name "*kernel_stats.csv" | sort); do
  echo "== $f"; grep -E "Name|dmcts" "$f"
done
