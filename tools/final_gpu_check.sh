cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${1:?usage: bash tools/final_gpu_check.sh OUTDIR}
mkdir -p $O
# every GPU step runs under a time limit of its own; the script stops at the first step that fails, times out or faults
timeout -k 10 2400 python -m pytest tests -x -q -m gpu > $O/pytest_gpu_full.log 2>&1; rc=$?
grep -v "^RCCL\|^HIP version\|^ROCm version\|^Hostname\|^Librccl" $O/pytest_gpu_full.log | tail -4 | tee $O/pytest_gpu.log
[ $rc -eq 0 ] || { echo "pytest exited $rc: stopping"; exit $rc; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_full.log 2>&1; rc=$?
tail -1 $O/smoke_full.log | tee $O/smoke.log
[ $rc -eq 0 ] || { echo "smoke exited $rc: stopping"; exit $rc; }
timeout -k 10 900 python bench.py --full > $O/bench_final.json 2> $O/bench_final.err; rc=$?
tail -c 800 $O/bench_final.json
exit $rc
