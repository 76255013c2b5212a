#!/bin/bash
# bench lines for the other BASELINE configs (not the headline): usage scripts/gpu_configs.sh <tag>
tag=${1:-run}
cd "$GRAFT_REPO_ROOT" 2>/dev/null || true
OUT=${OUT:-out}          # directory of the run's logs and bench lines
mkdir -p $OUT
python3 bench.py --full --batch 1 --height 256 --width 256 --steps 50 --warmup 10 --no-cpu-baseline > $OUT/cfg0_$tag.json 2> $OUT/cfg0_$tag.err && tail -2 $OUT/cfg0_$tag.err
python3 bench.py --full --batch 32 --height 720 --width 1280 --steps 5 --warmup 2 --no-cpu-baseline > $OUT/cfg2_$tag.json 2> $OUT/cfg2_$tag.err && tail -2 $OUT/cfg2_$tag.err
python3 bench.py --full --batch 16 --height 1080 --width 1920 --steps 3 --warmup 1 --no-cpu-baseline > $OUT/cfg4_$tag.json 2> $OUT/cfg4_$tag.err && tail -2 $OUT/cfg4_$tag.err
python3 bench.py --full --batch 8 --height 512 --width 512 --cin 6 --steps 20 --warmup 5 --no-cpu-baseline > $OUT/cfg1c6_$tag.json 2> $OUT/cfg1c6_$tag.err && tail -2 $OUT/cfg1c6_$tag.err
grep -h -o '"value": [0-9.]*\|"ms_per_step": [0-9.]*' $OUT/cfg*_$tag.json
