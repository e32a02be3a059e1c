# Round profiles: the full bench line, kernel trace + stats, then the PMC passes (each its own run, kernel-trace only).
#   bash tools/run_profiles.sh <tag>        outputs under $PROFILE_OUT/<tag>_* (default profile_out/)   (BENCH_ARGS="--precision bf16 --workload cfg4" for the bf16 path)
export TMPDIR=/tmp
tag=${1:-x}
export PROFILE_OUT=${PROFILE_OUT:-profile_out}
o=$PROFILE_OUT
mkdir -p $o
python bench.py --full $BENCH_ARGS > $o/${tag}_bench.log 2>&1
tail -1 $o/${tag}_bench.log > $o/${tag}_bench.json
bash tools/run_stats.sh ${tag} > /dev/null 2>&1
bash tools/run_pmc.sh ${tag}
dbs=$(for i in 1 2 3 4; do find $o/pmc_${tag}_$i -name "*.db" | head -1; done)
python tools/rocprof_pmc.py $dbs > $o/${tag}_pmc.md
tail -3 $o/${tag}_bench.json | cut -c1-300
