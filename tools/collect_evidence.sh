#!/usr/bin/env bash
# Reproduces the files under profiles/ for one round tag (run ON a GPU box, from the repo root):
#     tools/collect_evidence.sh r02a
# rocprofv3 wants a writable TMPDIR; counters are collected in their own passes (never together with sys/hip traces).
set -uo pipefail
TAG=${1:?round tag, e.g. r02a}
R=gpurun_out/$TAG
mkdir -p "$R"
export TMPDIR=/tmp
# FIESTA_REV=<commit> in the environment is recorded in the traffic summary (the GPU box has no .git)
# the parity suite with one JSON line per envelope comparison (the numbers DESIGN.md 3c quotes)
export FIESTA_ENVELOPE_LOG=$PWD/$R/envelope_reports.jsonl
rm -f "$FIESTA_ENVELOPE_LOG"
python -m pytest tests -q -m gpu --junitxml="$R/pytest_gpu.xml" > "$R/pytest_gpu.log" 2>&1
grep -aE "^(FAILED|ERROR)|[0-9]+ (passed|failed)" "$R/pytest_gpu.log" > "$R/pytest_gpu.txt"
unset FIESTA_ENVELOPE_LOG
# C2 headline as the driver runs it (the JSON line carries roofline + cpu_baseline incl. the full-size CPU leg, ~4 min) ...
python bench.py --full > "$R/bench_default.log" 2>&1
grep '^{"metric' "$R/bench_default.log" > "$R/bench_default.json"
# ... and the same GPU work under the kernel trace (without the 4-minute CPU leg)
rocprofv3 --kernel-trace --stats --output-format csv -d "$R/stats" -o bench -- python bench.py --full --no-cpu-full > "$R/bench_default_profiled.log" 2>&1
grep '^{"metric' "$R/bench_default_profiled.log" > "$R/bench_default_profiled.json"
# HBM traffic of UpdateESDF's kernels: two PMC passes, calibrated inside the same runs (tools/pmc_traffic.py)
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d "$R/pmc_$C" -o bench -- \
    python bench.py --steps 3 --warmup 1 --no-cpu-baseline > "$R/pmc_$C.log" 2>&1
done
python tools/pmc_traffic.py "$R/pmc_FETCH_SIZE" "$R/pmc_WRITE_SIZE" k_nn_ > "$R/pmc_traffic_cells.json"   # (r05: the cell transform serves C2)
# ... and the envelope passes on the same scene (--engine envelope), so that both transforms have their traffic on record
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d "$R/pmcE_$C" -o bench -- \
    python bench.py --steps 3 --warmup 1 --no-cpu-baseline --engine envelope > "$R/pmcE_$C.log" 2>&1
done
python tools/pmc_traffic.py "$R/pmcE_FETCH_SIZE" "$R/pmcE_WRITE_SIZE" k_ft_ > "$R/pmc_traffic_ft.json"
# issue / wait / LDS counters of the same command
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY \
  --output-format csv -d "$R/pmc_SQ" -o bench -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline > "$R/pmc_SQ.log" 2>&1
rocprofv3 --kernel-trace --pmc SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE \
  --output-format csv -d "$R/pmc_LDS" -o bench -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline > "$R/pmc_LDS.log" 2>&1
# the other scene, the other engine, the other configurations
python bench.py --full --engine envelope --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_c2_envelope.json"
python bench.py --workload queries 2>&1 | grep '^{"metric' > "$R/bench_queries.json"
python bench.py --full --scene surfaces --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_c2_surfaces.json"
python bench.py --full --engine rounds --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_c2_rounds.json"
python bench.py --full --engine rounds --scene surfaces --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_c2_surfaces_rounds.json"
python bench.py --full --engine levels --no-cpu-baseline --steps 3 --warmup 1 2>&1 | grep '^{"metric' > "$R/bench_c2_levels.json"
# C2-partial: 27 % of the map (32^3 blocks) never observed -> r06: the masked transform (mask_kernels.hpp); the frontier rounds pinned beside it
python bench.py --full --unobserved 0.27 --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_c2_partial.json"
python bench.py --full --unobserved 0.27 --engine rounds --no-cpu-baseline --steps 5 2>&1 | grep '^{"metric' > "$R/bench_c2_partial_rounds.json"
rocprofv3 --kernel-trace --stats --output-format csv -d "$R/stats_partial" -o partial -- python bench.py --full --unobserved 0.27 --no-cpu-baseline --steps 10 > "$R/c2_partial_profiled.log" 2>&1
python tools/density_range.py > "$R/density_range.json" 2> "$R/density_range.err"
python bench.py --workload c3 --steps 20 --warmup 4 2>&1 | grep '^{"metric' > "$R/bench_c3.json"
python bench.py --workload c3 --steps 20 --warmup 4 --engine rounds --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_c3_rounds.json"
python bench.py --workload c4 --steps 40 --warmup 5 2>&1 | grep '^{"metric' > "$R/bench_c4.json"
python bench.py --workload c4 --steps 40 --warmup 5 --engine rounds --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_c4_rounds.json"
python tools/dev/floor_latency.py > "$R/floor_latency.txt" 2>&1
# kernel stats of the sensor-rate configurations (level engine: k_level_run; hand-over: k_relax_q)
rocprofv3 --kernel-trace --stats --output-format csv -d "$R/stats_c3" -o c3 -- python bench.py --workload c3 --steps 20 --warmup 4 --no-cpu-baseline > "$R/c3_profiled.log" 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d "$R/stats_c4" -o c4 -- python bench.py --workload c4 --steps 40 --warmup 5 --no-cpu-baseline > "$R/c4_profiled.log" 2>&1
python bench.py --full --gpus 1 --force-sharded --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_sharded_1rank.json"
python bench.py --delta-sweep --no-cpu-baseline 2>&1 | grep -E "^\{" > "$R/delta_sweep.json"
# config-5-sized pieces on one GPU: one 1024^3 shard through the native group, two of them multiplexed (2048 x 1024 x 1024)
python bench.py --full --gpus 1 --force-sharded --grid 1024 --steps 5 --warmup 1 --no-cpu-baseline 2>&1 | grep '^{"metric' > "$R/bench_1024_one_shard.json"
python tools/c5_smoke.py > "$R/c5_two_shards_bulk.json" 2> "$R/c5_smoke.err"
# the parity suite twice more (ties inside a level fall differently from run to run: is any test at its margin?)
for k in 2; do python -m pytest tests -q -m gpu 2>&1 | grep -aE "^(FAILED|ERROR)|[0-9]+ (passed|failed)" >> "$R/pytest_gpu.txt"; done
# copy what is to be judged into profiles/ (gpurun_out/ is scratch)
cp "$R/stats/bench_kernel_stats.csv" "profiles/${TAG}_bench_kernel_stats_default.csv"
cp "$R/stats_partial/partial_kernel_stats.csv" "profiles/${TAG}_c2_partial_kernel_stats.csv"
for f in bench_default bench_default_profiled delta_sweep bench_c2_envelope bench_queries pmc_traffic_cells bench_c2_surfaces bench_c2_rounds bench_c2_surfaces_rounds bench_c2_levels bench_c2_partial bench_c2_partial_rounds density_range \
         bench_c3 bench_c3_rounds bench_c4 bench_c4_rounds bench_sharded_1rank bench_1024_one_shard c5_two_shards_bulk pmc_traffic_ft; do
  cp "$R/$f.json" "profiles/${TAG}_$f.json"
done
cp "$R/floor_latency.txt" "profiles/${TAG}_floor_latency.txt"
cp "$R/pytest_gpu.txt" "profiles/${TAG}_pytest_gpu.txt"
cp "$R/envelope_reports.jsonl" "profiles/${TAG}_envelope_reports.jsonl"
cp "$R/stats_c3/c3_kernel_stats.csv" "profiles/${TAG}_c3_kernel_stats.csv"
cp "$R/stats_c4/c4_kernel_stats.csv" "profiles/${TAG}_c4_kernel_stats.csv"
for C in FETCH_SIZE WRITE_SIZE SQ LDS; do
  cp "$R/pmc_$C/bench_counter_collection.csv" "profiles/${TAG}_pmc_${C}_counter_collection.csv"
done
python -c "import __graft_entry__ as g; g.smoke()" > "$R/smoke.txt" 2>&1; echo "smoke rc=$?" >> "$R/smoke.txt"
find "$R" -name "*.db" -delete 2>/dev/null
echo "evidence for $TAG written in $R (gpurun merges gpurun_out/ back; tools/copy_evidence.sh $TAG copies the judged files into profiles/)"
