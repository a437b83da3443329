#!/bin/bash
# Everything the round's evidence needs, in one GPU-box call:  bash tools/round_artifacts.sh r03 <output directory>
#   1. regenerate the autotune cache over every bench workload / dtype (tools/regen_cache.sh, its bench lines in that script's folder)
#   2. the full GPU test suite with that cache (summary in <output directory>)
#   3. rocprofv3 kernel stats + FETCH_SIZE / WRITE_SIZE passes of the default bench (tools/profile_round.sh) -> profiles/<tag>_*
#   4. one traced step (timeline + per-queue accounting, tools/trace_step.sh) and the `--full` bench line with its per-launch table
#      (<output directory>/<tag>_launches.txt, <tag>_bench_full.json); this script's logs go to <output directory> too
tag=${1:-r03}
dst=${2:?usage: bash tools/round_artifacts.sh <tag> <output directory>}  # this script's own logs, test summary, launch table and bench line
mkdir -p "$dst"
export FALNET_COMMIT=${FALNET_COMMIT:-unknown}
bash tools/regen_cache.sh $tag > "$dst/${tag}_regen.log" 2>&1
python -m pytest tests -m gpu -q 2>&1 | tail -8 > "$dst/${tag}_pytest.txt"
bash tools/profile_round.sh $tag > "$dst/${tag}_profile.log" 2>&1
bash tools/trace_step.sh $tag
python bench.py --full --launch-table "$dst/${tag}_launches.txt" > "$dst/${tag}_bench_full.json" 2> "$dst/${tag}_bench_full.err"
tail -3 "$dst/${tag}_pytest.txt"; tail -9 "$dst/${tag}_regen.log" | cut -c1-300; tail -1 "$dst/${tag}_bench_full.json" | cut -c1-600
