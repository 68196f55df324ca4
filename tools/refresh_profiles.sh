set -e
R=$GRAFT_REPO_ROOT
O=${1:?usage: bash tools/refresh_profiles.sh OUTDIR}
mkdir -p $O && O=$(cd $O && pwd)
python3 $R/bench.py --full > $O/bench_default.json 2> $O/bench_default.log
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d /tmp/kt2048 -o r -- python3 $R/bench.py --no-cpu-baseline --no-roofline --no-graph --steps 10 --warmup 3 > $O/prof2048.log 2>&1
{ echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py ... --no-graph --steps 10 --warmup 3 (per-kernel totals via tools/rocpd_stats.py; 13 steps traced, times per step)"; python3 $R/tools/rocpd_stats.py $(find /tmp/kt2048 -name "*.db" | head -1) 13; } > $O/B2048_kernel_stats.txt
rocprofv3 --kernel-trace --stats -d /tmp/kt256 -o r -- python3 $R/bench.py --batch 256 --no-cpu-baseline --no-roofline --no-graph --steps 10 --warmup 3 > $O/prof256.log 2>&1
{ echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py ... --no-graph --steps 10 --warmup 3 (per-kernel totals via tools/rocpd_stats.py; 13 steps traced, times per step)"; python3 $R/tools/rocpd_stats.py $(find /tmp/kt256 -name "*.db" | head -1) 13; } > $O/B256_kernel_stats.txt
echo refreshed
