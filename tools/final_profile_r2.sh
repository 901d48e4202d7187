#!/bin/bash
# GPU-box job that regenerates everything under profiles/r2 (run once the kernels are final): bench lines, rocprofv3
# kernel-trace stats of the bench command, PMC passes (FETCH_SIZE / WRITE_SIZE in their own passes, SQ counters), sweeps.
set -e
O=gpurun_out/final_r2
mkdir -p $O
export TMPDIR=/tmp
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench_driver_cmd.json 2> $O/bench_driver_cmd.err
echo bench done
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o run -- python3 bench.py --full --steps 2048 --warmup 512 --repeats 5 --no-cpu-baseline > $O/bench_under_rocprof.json 2>/dev/null
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats20 -o run -- python3 bench.py --full --steps 20 --warmup 5 --repeats 200 --no-cpu-baseline > $O/bench20_under_rocprof.json 2>/dev/null
rocprofv3 --kernel-trace --output-format csv --pmc FETCH_SIZE -d $O/pmc_fetch -o run -- python3 bench.py --full --steps 1024 --warmup 512 --repeats 5 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --kernel-trace --output-format csv --pmc WRITE_SIZE -d $O/pmc_write -o run -- python3 bench.py --full --steps 1024 --warmup 512 --repeats 5 --no-cpu-baseline > /dev/null 2>&1
PMC="SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_INST_LDS"
rocprofv3 --kernel-trace --output-format csv --pmc $PMC -d $O/pmc_sq_4096 -o run -- python3 bench.py --full --steps 1024 --warmup 512 --repeats 5 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --kernel-trace --output-format csv --pmc $PMC -d $O/pmc_sq_65536 -o run -- python3 bench.py --full --steps 128 --warmup 64 --roll 64 --repeats 5 --no-cpu-baseline --worlds 65536 --pool-factor 2 > /dev/null 2>&1
echo pmc done
for d in pmc_fetch pmc_write pmc_sq_4096 pmc_sq_65536; do python tools/pmc_summary.py $O/$d k_rollout3 > $O/$d.txt; done
: > $O/sweep.txt
for N in 16384 65536 262144; do
  R=64; if [ $N -ge 262144 ]; then R=16; fi
  echo "N=$N roll=$R" >> $O/sweep.txt
  python bench.py --full --no-cpu-baseline --worlds $N --roll $R --steps 512 --warmup 128 --repeats 5 --pool-factor 2 --scenarios device >> $O/sweep.txt
done
for R in 20 64 128 256; do
  echo "N=4096 roll=$R (steps per launch)" >> $O/sweep.txt
  python bench.py --full --no-cpu-baseline --roll $R --repeats 5 >> $O/sweep.txt
done
echo "per-step launches (cagym_step_autoreset)" >> $O/sweep.txt
python bench.py --full --no-cpu-baseline --per-step-launch --steps 1024 --warmup 128 --repeats 5 >> $O/sweep.txt
echo "cfg2 4096x4 NonCooperative" >> $O/sweep.txt
python bench.py --full --no-cpu-baseline --config cfg2 --repeats 5 >> $O/sweep.txt
echo "2048x20 RVO (maxNeighbors 20)" >> $O/sweep.txt
python bench.py --full --no-cpu-baseline --worlds 2048 --agents 20 --roll 256 --repeats 5 >> $O/sweep.txt
echo sweep done
python bench.py --full --config cfg4 --steps 200 --warmup 50 > $O/bench_cfg4.json 2> $O/bench_cfg4.err
python bench.py --full --config cfg5 --steps 200 --warmup 50 > $O/bench_cfg5.json 2> $O/bench_cfg5.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_cfg4 -o run -- python3 bench.py --full --config cfg4 --steps 200 --warmup 50 --repeats 5 --no-cpu-baseline > $O/bench_cfg4_under_rocprof.json 2>/dev/null
python tools/ga3c_ab.py > $O/ga3c_ab.txt 2>&1
hipcc --offload-arch=gfx950 -O3 -Wno-unused-result -o /tmp/mfma_rate tools/micro/mfma_rate.hip 2>/dev/null && /tmp/mfma_rate > $O/mfma_rate.txt
echo rows done
CAGYM_BENCH_BACKEND=gloo python bench.py --full --gpus 2 --steps 512 --warmup 64 --roll 64 --repeats 5 --no-cpu-baseline > $O/rehearsal_2ranks_gloo.json 2> $O/rehearsal_2ranks_gloo.err
echo rehearsal done
python tools/wave_trace.py > $O/wave_trace_4096.txt 2>&1
python tools/launch_cost.py > $O/launch_cost.txt 2>&1
python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
echo smoke done
