#!/bin/bash
# A/B of two builds of the library on the headline bench (diagnostics; run on the GPU box)
# usage: tools/ab.sh <alt_lib.so> [tag]
set -e
O=${OUT_DIR:-exp_out}  # where the JSON lines go
mkdir -p $O
T=${2:-alt}
python bench.py --full --no-cpu-baseline > $O/base.json
CAGYM_LIB=$1 python bench.py --full --no-cpu-baseline > $O/$T.json
python bench.py --full --no-cpu-baseline --worlds 65536 --steps 512 --warmup 128 --pool-factor 2 > $O/base64k.json
CAGYM_LIB=$1 python bench.py --full --no-cpu-baseline --worlds 65536 --steps 512 --warmup 128 --pool-factor 2 > $O/${T}64k.json
python - <<PY
import json
for f in ("base", "$T", "base64k", "${T}64k"):
    d = json.load(open("$O/%s.json" % f))
    print(f, "%.1f M env-steps/s" % (d["value"] / 1e6), "launch %.3f ms" % d["roofline"]["launch_ms"], "frac %.4f" % d["roofline"]["frac"])
PY
