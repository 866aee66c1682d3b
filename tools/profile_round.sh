# Profiles committed under profiles/ (run on the GPU box from the repo root):
#   1. kernel trace + stats of the full bench (CSV summary + SQLite)
#   2. FETCH_SIZE and WRITE_SIZE passes (separate: TCC slots), for HBM traffic
# Output goes to $ZK_PROF_OUT (default: prof_out/ in the repo root).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=${ZK_PROF_OUT:-$R/prof_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats -o run -- python3 $R/bench.py --full --no-cpu-baseline --no-msm --steps 5 > $O/prof_stats.log 2>&1
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof_db -o run -- python3 $R/bench.py --full --no-cpu-baseline --steps 5 > $O/prof_db.log 2>&1
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_fetch -o run -- python3 $R/bench.py --full --no-cpu-baseline --no-msm --steps 3 --warmup 1 > $O/pmc_fetch.log 2>&1
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE -d $O/pmc_write -o run -- python3 $R/bench.py --full --no-cpu-baseline --no-msm --steps 3 --warmup 1 > $O/pmc_write.log 2>&1
