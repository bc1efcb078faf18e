#!/bin/bash
# Everything the round's committed evidence comes from, in one GPU call.  usage: OUT=<output dir> bash profiles/scripts/final_round.sh <tag>   (e.g. r02)
TAG=${1:-r02}
R=$GRAFT_REPO_ROOT
cd $R
export OUT=$(realpath "${OUT:?set OUT to the output directory}"); mkdir -p $OUT
python -m pytest tests -m gpu -q > $OUT/${TAG}_gputests.log 2>&1; tail -2 $OUT/${TAG}_gputests.log
# HBM counters first (bench.py only accepts a PMC summary taken on the same kernel sources)
bash profiles/scripts/pmc_bench.sh 128 $OUT/${TAG}_pmc_bench.json > $OUT/${TAG}_pmc_bench.txt 2>&1
cp $OUT/${TAG}_pmc_bench.json profiles/${TAG}_pmc_bench.json
cd $R
python bench.py --full > $OUT/${TAG}_bench_final.json 2> $OUT/${TAG}_bench_final.err; tail -c 600 $OUT/${TAG}_bench_final.json
bash profiles/scripts/trace_bench.sh ${TAG}_bench_final
cd $R
for b in 16 32 64; do python bench.py --full --batch $b --steps 3 --no-cpu-baseline 2>/dev/null | grep '^{' > $OUT/${TAG}_bench_b$b.json; done
python bench.py --full --precision native --steps 3 --no-cpu-baseline 2>/dev/null | grep '^{' > $OUT/${TAG}_bench_native.json
python tests/gpu_gemm_bench.py 2>&1 | grep -v amdgpu > $OUT/${TAG}_gemm_shapes.txt
timeout 300 python tests/gpu_config5.py 2>&1 | grep -v amdgpu > $OUT/${TAG}_config5.log
timeout 400 python tests/gpu_config3.py 21 32 32 2>&1 | grep -v amdgpu > $OUT/${TAG}_config3.log
