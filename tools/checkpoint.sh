#!/bin/bash
# tools/checkpoint.sh <tag> [out] — the round-end sequence on the GPU box: the GPU test tier, then the full bench record (default out: checkpoints/<tag>)
tag=${1:-r04/g}
out=${2:-checkpoints/$tag}
mkdir -p $out
(time python -m pytest tests -m gpu -x -q) > $out/gputests.log 2>&1
grep -E "passed|failed|error" $out/gputests.log | tail -3
python bench.py --steps 5 --warmup 2 --full --detail $out/bench_detail.json > $out/bench.json 2> $out/bench.err
tail -c 300 $out/bench.err
echo "bench line: $(tail -n 1 $out/bench.json | wc -c) bytes (the line's bound: 6000)"
python tools/show_bench.py $out/bench_detail.json
