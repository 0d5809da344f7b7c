#!/bin/bash
# OUT/head_* (written by tools/run_head_profiles.sh OUT) -> profiles/rNN_*  :  tools/collect_head_profiles.sh r03 OUT
set -e
R=${1:-r03}; O=$(cd "${2:?usage: tools/collect_head_profiles.sh rNN OUT}" && pwd); cd "$(dirname "$0")/.."
cp $O/head_bench.json profiles/${R}_bench_dp1.json
cp $O/head_kernel_stats.csv profiles/${R}_bench_dp1_kernel_stats.csv
cp $O/head_kernel_stats_serial.csv profiles/${R}_bench_dp1_kernel_stats_serial.csv
cp $O/head_bench_dp_size1.json profiles/${R}_bench_dp_size1.json
cp $O/head_bench_dp_size1_bf16wire.json profiles/${R}_bench_dp_size1_bf16wire_4buckets.json
cp $O/other_configs.jsonl profiles/${R}_bench_other_configs.jsonl
cp $O/head_dense.jsonl profiles/${R}_dense_layer_microbench.jsonl
cp $O/head_gpu_idle_gaps.txt profiles/${R}_gpu_idle_gaps.txt
cp $O/head_infonce.jsonl profiles/${R}_infonce_microbench.jsonl
cp $O/head_layer_times_serial.txt profiles/${R}_layer_times_serial.txt
cp $O/head_overlap_modes.txt profiles/${R}_overlap_modes.txt
cp $O/head_pmc_hbm_traffic.txt profiles/${R}_pmc_hbm_traffic.txt
cp $O/head_spot.json profiles/${R}_spot_branch.json
cp $O/head_gemm.jsonl profiles/${R}_gemm_bf16_microbench.jsonl
cp $O/head_proj_head.jsonl profiles/${R}_proj_head_microbench.jsonl
cp $O/head_step_stamps.txt profiles/${R}_step_stamps.txt
cp $O/head_kernel_traffic.json profiles/kernel_traffic.json
ls -la profiles/${R}_* | wc -l
