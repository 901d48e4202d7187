#!/bin/bash
# Same-box A/B of `python bench.py [args]` with the libraries taken in turn, round after round (tools/ab.sh runs each library once;
# a gain of a few per cent needs the box's drift taken out).  The base library is run TWICE per round (sets base1 / base2): the
# difference of their medians is the spread a library shows against itself; a gain counts when it exceeds three times that.
# usage: tools/ab_interleaved.sh <rounds> "<bench args>" <base.so> <alt.so | shipped> [...]     ("shipped" = the in-tree library)
set -o pipefail
R=$1; ARGS=$2; BASE=$3; shift 3
O=${OUT_DIR:-exp_out}/ab_interleaved  # where the JSON lines go
mkdir -p $O
N=0; NAMES="base1"
for L in "$@"; do N=$((N + 1)); NAMES="$NAMES alt$N"; done
NAMES="$NAMES base2"
for rep in $(seq 1 $R); do
  i=0
  for T in $NAMES; do
    case $T in
      base1|base2) export CAGYM_LIB=$BASE;;
      *) i=$((i + 1)); L=${!i}; if [ $L = shipped ]; then unset CAGYM_LIB; else export CAGYM_LIB=$L; fi;;
    esac
    timeout -k 10 300 python bench.py $ARGS > $O/${T}_$rep.json 2>/dev/null || exit 1
  done
done
python - "$@" <<PY
import json, statistics as st, sys
names = "$NAMES".split()
label = dict(zip([n for n in names if n.startswith("alt")], sys.argv[1:]), base1="$BASE", base2="$BASE")
v = {T: [json.load(open("$O/%s_%d.json" % (T, r)))["value"] / 1e6 for r in range(1, $R + 1)] for T in names}
print("python bench.py $ARGS: $R rounds, the libraries in turn; M env-steps/s")
for T in names:
    print("%-6s %-40s median %.2f min %.2f max %.2f |" % (T, label[T][-40:], st.median(v[T]), min(v[T]), max(v[T])), " ".join("%.1f" % x for x in v[T]))
base = st.median(v["base1"] + v["base2"])
spread = abs(st.median(v["base1"]) - st.median(v["base2"]))
print("base (both sets) median %.2f; spread of the two sets' medians %.2f; bar = 3 x spread = %.2f" % (base, spread, 3 * spread))
for T in names:
    if T.startswith("alt"):
        print("%-6s %-40s %+.2f M against the base (%+.2f %%)" % (T, label[T][-40:], st.median(v[T]) - base, 100 * (st.median(v[T]) / base - 1)))
PY
