#!/bin/bash
# Round-2 measurement pass on the GPU box: full bench line, the other named configurations, rocprofv3 kernel stats
# (cfg B and C, eager launches) and the PMC passes.  The bench lines and PMC summaries land under the output directory
# (relative to the repository root); the summaries to keep are copied into profiles/ afterwards.
#   scripts/r02_collect.sh <out dir>
out=${1:?usage: scripts/r02_collect.sh <out dir>}
cd $GRAFT_REPO_ROOT
mkdir -p "$out"
python bench.py --full --steps 30 --warmup 5 > "$out"/r02_bench_default.json 2> "$out"/r02_bench_default.err || echo "default bench failed"
for c in A C Cp D ref; do
  python bench.py --full --config $c --steps 20 --warmup 5 --cpu-budget 8 > "$out"/r02_bench_cfg$c.json 2> "$out"/r02_bench_cfg$c.err || echo "bench $c failed"
done
scripts/prof_step.sh r02B > /dev/null 2>&1
scripts/prof_step.sh r02C --config C > /dev/null 2>&1
scripts/pmc_family.sh B "$out"/r02_pmc_family_cfgB.json > "$out"/pmcB.log 2>&1
scripts/pmc_family.sh C "$out"/r02_pmc_family_cfgC.json > "$out"/pmcC.log 2>&1
ls -la "$out"/r02_*
