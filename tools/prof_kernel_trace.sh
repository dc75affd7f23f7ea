# Kernel-trace statistics of every kernel of the full bench line (headline + sub-records, no CPU baseline).
# usage (GPU box): bash tools/prof_kernel_trace.sh [output directory, default profile_out/kernel_trace]
set -e
cd "$(dirname "$0")/.."
out=${1:-profile_out/kernel_trace}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $out/bench.log 2>&1
tail -2 $out/bench.log
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kt -- python bench.py --full --no-cpu-baseline > $out/kt.log 2>&1
find $out -name "*stats*" | head
