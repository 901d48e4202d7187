#!/bin/bash
# headline bench for several alternative libraries: tools/abn.sh lib1.so lib2.so ...
O=${OUT_DIR:-exp_out}  # where the JSON lines go
mkdir -p $O
for L in "$@"; do
  T=$(basename $L .so)
  CAGYM_LIB=$L python bench.py --full --no-cpu-baseline > $O/$T.json || exit 1
  CAGYM_LIB=$L python bench.py --full --no-cpu-baseline --worlds 65536 --steps 512 --warmup 128 --pool-factor 2 > $O/${T}_64k.json || exit 1
  python - <<PY
import json
for f in ("$T", "${T}_64k"):
    d = json.load(open("$O/%s.json" % f))
    print(f, "%.1f M env-steps/s" % (d["value"] / 1e6), "launch %.3f ms" % d["roofline"]["launch_ms"], "frac %.4f" % d["roofline"]["frac"])
PY
done
