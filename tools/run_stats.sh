# rocprofv3 kernel trace + stats of a plain bench run (warm-up + timed steps of the headline workload only); DB under $PROFILE_OUT/prof_<tag>/
export TMPDIR=/tmp
tag=${1:-x}
o=${PROFILE_OUT:-profile_out}
mkdir -p $o
rocprofv3 --kernel-trace --stats -d $o/prof_${tag} -o p -- python bench.py --steps 5 --warmup 2 $BENCH_ARGS > $o/prof_${tag}_bench.log 2>&1
db=$(find $o/prof_${tag} -name "*.db" | head -1)
python tools/rocprof_summary.py $db $o/prof_${tag}_summary.md
tail -1 $o/prof_${tag}_bench.log > $o/prof_${tag}_bench.json
head -20 $o/prof_${tag}_summary.md
