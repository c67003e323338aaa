# kernel trace (csv) of a short bench run (--full) -> $PROF_OUT/NAME (default prof_out/):  bash tools/prof_trace.sh NAME [bench args]
NAME=${1:-trace}; shift
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${PROF_OUT:-prof_out}; mkdir -p $OUT
python bench.py --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$NAME -o run -- python3 bench.py --full --steps 4 --warmup 2 --no-cpu-baseline "$@" > $OUT/$NAME.log 2>&1
find $OUT/$NAME -name "*kernel_trace.csv" | head -1 | xargs -I{} python tools/timeline.py {} 2 > $OUT/$NAME.timeline.txt 2>&1
head -50 $OUT/$NAME.timeline.txt
