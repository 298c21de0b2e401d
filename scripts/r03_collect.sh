#!/bin/bash
# Round-3 measurement pass on the GPU box: full bench line, the other named configurations, rocprofv3 kernel stats
# (cfg B, C and D, eager launches) and the PMC passes (cfg B and C).  The bench lines and PMC summaries land under the
# output directory (relative to the repository root); the summaries to keep are copied into profiles/ afterwards
# (bench.py --full reads profiles/r03_pmc_family_cfg<id>.json for roofline.traffic).
#   scripts/r03_collect.sh <out dir>
out=${1:?usage: scripts/r03_collect.sh <out dir>}
cd $GRAFT_REPO_ROOT
mkdir -p "$out"
scripts/pmc_family.sh B "$out"/r03_pmc_family_cfgB.json > "$out"/pmcB.log 2>&1
scripts/pmc_family.sh C "$out"/r03_pmc_family_cfgC.json > "$out"/pmcC.log 2>&1
mkdir -p profiles && cp "$out"/r03_pmc_family_cfgB.json "$out"/r03_pmc_family_cfgC.json profiles/ 2>/dev/null
scripts/prof_step.sh r03B > /dev/null 2>&1
scripts/prof_step.sh r03C --config C > /dev/null 2>&1
scripts/prof_step.sh r03D --config D > /dev/null 2>&1
python bench.py --full > "$out"/r03_bench_default.json 2> "$out"/r03_bench_default.err || echo "default bench failed"
for c in A C Cp D ref; do
  python bench.py --full --config $c --steps 20 --warmup 5 --cpu-budget 8 --no-accuracy > "$out"/r03_bench_cfg$c.json 2> "$out"/r03_bench_cfg$c.err || echo "bench $c failed"
done
ls -la "$out"/r03_*
