#!/usr/bin/env bash
# One box, the evidence of a round:
#   1. the WHOLE GPU test suite (also writes gpurun_out/parity_latents.json -> profiles/, which bench.py embeds in its line)
#   2. HBM-traffic PMC passes (attention + regional kernels) for the current kernel sources
#   3. the default bench line (train + regional halves, cpu baselines)
#   4. rocprofv3 --kernel-trace --stats of BOTH halves
#   5b. the shipped 1024x2048 example, 5. the JPEG-fed training step, 2b. PMC of the halo convolution / probability kernels,
#   6. the configs[3] fusion line   (least essential last: the call's time limit is whatever GPU budget is left)
# Copy gpurun_out/<tag>_* into profiles/ afterwards.        bash tools/final_gpu_run.sh <tag>
set -u
TAG="${1:-r06}"
ROOT="${GRAFT_REPO_ROOT:-$(pwd)}"
cd "$ROOT"
O="$ROOT/gpurun_out"; mkdir -p "$O"
rm -f "$O/parity_latents.json"
echo "== 1. full GPU test suite"
timeout ${TESTS_TIMEOUT:-1500} python -m pytest tests -m gpu -q -rP --durations=12 > "$O/${TAG}_gpu_tests_full.log" 2>&1
echo "rc=$?"
# the [parity] / smoke lines of every test (passed ones included), and the summary
grep -E "^\[parity\]|^smoke:" "$O/${TAG}_gpu_tests_full.log" | sort -u > "$O/${TAG}_gpu_tests_parity_lines.txt"
sed -n '/slowest 12 durations/,$p' "$O/${TAG}_gpu_tests_full.log" | grep -v "^\[parity\]" | tail -40 > "$O/${TAG}_gpu_tests.log"
tail -16 "$O/${TAG}_gpu_tests.log" | cut -c1-200; wc -l "$O/${TAG}_gpu_tests_parity_lines.txt"; rm -f "$O/${TAG}_gpu_tests_full.log"
if [ -f "$O/parity_latents.json" ]; then cp "$O/parity_latents.json" profiles/parity_latents.json; echo "profiles/parity_latents.json refreshed: $(python -c "import json; print(len(json.load(open('profiles/parity_latents.json'))['cases']), 'cases')")"; fi
# the HBM-traffic PMC passes belong to the attention kernel sources (bench.PMC_SOURCE_FILES): re-collected only when those changed
if python -c "import json,bench,sys; sys.exit(0 if json.load(open('profiles/pmc_traffic.json')).get('source_sha16') == bench.kernel_source_fingerprint() else 1)" 2>/dev/null \
   && [ -z "${FORCE_PMC:-}" ]; then
  echo "== 2. PMC: profiles/pmc_traffic.json matches the attention kernel sources in the tree, passes not repeated"
else
echo "== 2. PMC (attn,region): sq1 sq2 fetch write"
PMC_BENCH_ARGS="--ref 0" bash tools/pmc_collect.sh attn,region > "$O/${TAG}_pmc_run.log" 2>&1
cp "$O/pmc_attn,region.txt" "$O/${TAG}_pmc_attention_region_kernels.txt" 2>/dev/null
python tools/pmc_traffic.py /tmp/pmc_fetch /tmp/pmc_write > "$O/${TAG}_pmc_traffic.json" 2>> "$O/${TAG}_pmc_run.log"
if python -c "import json,sys; d=json.load(open('$O/${TAG}_pmc_traffic.json')); sys.exit(0 if d.get('kernels') else 1)"; then
  cp "$O/${TAG}_pmc_traffic.json" profiles/pmc_traffic.json; echo "pmc_traffic.json refreshed: $(python -c "import json; print(list(json.load(open('profiles/pmc_traffic.json'))['kernels']))")"
else echo "PMC FAILED"; tail -5 "$O/${TAG}_pmc_run.log"; fi
fi
echo "== 3. default bench"
timeout 900 python bench.py --full --steps 20 --warmup 5 > "$O/${TAG}_bench_train_n1.json" 2> "$O/${TAG}_bench_train_n1.err"
cp "$O/bench_full.json" "$O/${TAG}_bench_train_n1_full_record.json" 2>/dev/null     # the verbose record (kernel tables, per-case parity) of that line
grep -E "timed region|captured" "$O/${TAG}_bench_train_n1.err" | cut -c1-330; wc -c "$O/${TAG}_bench_train_n1.json"; cut -c1-400 "$O/${TAG}_bench_train_n1.json"
cd /tmp && export TMPDIR=/tmp
echo "== 4. rocprofv3 kernel stats: train"
rm -rf /tmp/prof
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -o b -- python "$ROOT/bench.py" --full --steps 6 --warmup 2 --no-cpu-baseline --no-regional \
    > "$O/${TAG}_bench_train_under_rocprof.json" 2> "$O/${TAG}_rocprof.err"
f=$(find /tmp/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && head -100 "$f" > "$O/${TAG}_rocprofv3_kernel_stats_bench_train.csv"
echo "== rocprofv3 kernel stats: regional"
rm -rf /tmp/prof2
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof2 -o b -- python "$ROOT/bench.py" --full --mode regional --steps 3 --warmup 1 --no-cpu-baseline \
    > "$O/${TAG}_bench_regional_under_rocprof.json" 2> "$O/${TAG}_rocprof_regional.err"
f=$(find /tmp/prof2 -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && head -100 "$f" > "$O/${TAG}_rocprofv3_kernel_stats_bench_regional.csv"
cd "$ROOT"
grep -E "attn_bwd_dkdv(_pipe)?_kernelIDF16_Li40|conv3x3_(nhwc|halo)_kernel|gn_col_kernel" "$O/${TAG}_rocprofv3_kernel_stats_bench_train.csv" | cut -c1-160 | head -8
grep -E "attn_fwd_kernelIDF16_Li40|region_attn_kernel|gn_col_kernel" "$O/${TAG}_rocprofv3_kernel_stats_bench_regional.csv" | cut -c1-160 | head -8
cut -c1-200 "$O/${TAG}_bench_train_under_rocprof.json"; cut -c1-200 "$O/${TAG}_bench_regional_under_rocprof.json"
echo "== 5b. the reference's shipped regional example, 1024x2048"
timeout 400 python bench.py --full --mode regional --height 1024 --width 2048 --steps 2 --warmup 1 > "$O/${TAG}_bench_regional_1024x2048.json" 2> "$O/${TAG}_bench_regional_1024x2048.err"
cp "$O/bench_full.json" "$O/${TAG}_bench_regional_1024x2048_full_record.json" 2>/dev/null; cut -c1-260 "$O/${TAG}_bench_regional_1024x2048.json"
echo "== 5. train step fed by the JPEG data pipeline (SURVEY 8(f).4)"
timeout 150 python bench.py --full --steps 20 --warmup 5 --data jpeg --no-cpu-baseline --no-regional > "$O/${TAG}_bench_train_jpeg.json" 2> "$O/${TAG}_bench_train_jpeg.err"
tail -1 "$O/${TAG}_bench_train_jpeg.err"; cut -c1-200 "$O/${TAG}_bench_train_jpeg.json"
echo "== 2b. PMC of the halo convolution (one shape: B4 320->320 64x64) and of the materialised-probability kernels"
PMC_BENCH_ARGS="--ref 0" bash tools/pmc_collect.sh conv1,probs > "$O/${TAG}_pmc_conv_run.log" 2>&1
cp "$O/pmc_conv1,probs.txt" "$O/${TAG}_pmc_conv_halo_and_probs_kernels.txt" 2>/dev/null; grep -A16 "conv3x3_halo_kernel f16" "$O/${TAG}_pmc_conv_halo_and_probs_kernels.txt" | head -40
echo "== 6. configs[3]: gradient fusion of 14 synthetic ED-LoRAs"
timeout 420 python bench.py --full --mode fusion --concepts 14 --steps 2 --warmup 1 > "$O/${TAG}_bench_fusion.json" 2> "$O/${TAG}_bench_fusion.err"
echo "rc=$?"; cp "$O/bench_full.json" "$O/${TAG}_bench_fusion_full_record.json" 2>/dev/null; grep "fusion pass" "$O/${TAG}_bench_fusion.err"; cut -c1-300 "$O/${TAG}_bench_fusion.json"
