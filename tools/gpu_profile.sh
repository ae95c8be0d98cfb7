# Full measurement set on the GPU box (one call): parity tests, a kernel-trace
# --stats profile, the --pmc passes that feed profiles/pmc_latest.json, and the
# bench line (with the CPU baseline).  Counter passes are separate runs with
# --kernel-trace only (no sys/runtime trace), each under its own time limit.
set -u
TAG=${TAG:-r02c}
OUT=gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
if [ "${PYTEST:-1}" = 1 ]; then
  timeout -k 10 700 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -2 $OUT/pytest_gpu.log
  [ $rc -eq 0 ] || exit $rc
fi
# (PMC passes: 8 steps after 4 warm-up ones, so the prefilter's listed items
# -- built from the previous detect -- are in steady state; every bench run
# here also takes bench.py's default --settle steps first, as the driver's
# does, so the per-launch averages are those of a device at steady clocks.)
# The profiled runs skip the bench's secondary lines (--no-variants): their
# gated / cadence-skipped launches would otherwise dilute the per-launch
# averages of the headline workload's kernels.
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/stats -o run --output-format csv -- \
    python bench.py --steps 20 --warmup 3 --no-cpu --no-variants > $OUT/prof_stats.log 2>&1
rc=$?; echo "stats rc=$rc"; [ $rc -eq 0 ] || exit $rc
i=0
for set in "FETCH_SIZE" "WRITE_SIZE" \
           "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_SALU" \
           "SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_TRANS_F64 SQ_ACTIVE_INST_VALU"; do
  i=$((i+1))
  timeout -k 10 120 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $OUT/pmc_p$i -o run -- \
      python bench.py --steps 8 --warmup 4 --no-cpu --no-variants > $OUT/pmc_p$i.log 2>&1
  rc=$?; echo "pmc pass $i rc=$rc"; [ $rc -eq 0 ] || exit $rc
done
python tools/pmc_roofline.py $OUT/pmc_latest.json $OUT/pmc_p1 $OUT/pmc_p2 $OUT/pmc_p3 $OUT/pmc_p4
cp $OUT/pmc_latest.json profiles/pmc_latest.json
# K4' on its own (BSA_K24=0: K2 and K4' as two launches): the propagation
# kernel's standalone duration and HBM bytes, which the fused default launch
# only bounds (VERDICT r04 missing #3); same passes, kernel-trace only
if [ "${K24PASS:-1}" = 1 ]; then
  timeout -k 10 300 env BSA_K24=0 rocprofv3 --kernel-trace --stats -d $OUT/k24off_stats -o run --output-format csv -- \
      python bench.py --steps 20 --warmup 3 --no-cpu --no-variants > $OUT/k24off_stats.log 2>&1
  rc=$?; echo "k24=0 stats rc=$rc"; [ $rc -eq 0 ] || exit $rc
  j=0
  for set in "FETCH_SIZE" "WRITE_SIZE"; do
    j=$((j+1))
    BSA_K24=0 timeout -k 10 120 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $OUT/k24off_p$j -o run -- \
        python bench.py --steps 8 --warmup 4 --no-cpu --no-variants > $OUT/k24off_p$j.log 2>&1
    rc=$?; echo "k24=0 pmc pass $j rc=$rc"; [ $rc -eq 0 ] || exit $rc
  done
  python tools/pmc_roofline.py $OUT/pmc_k24off.json $OUT/k24off_p1 $OUT/k24off_p2
  cp $OUT/pmc_k24off.json profiles/pmc_k24off.json
fi
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 > $OUT/bench.json 2> $OUT/bench.err
rc=$?; echo "bench rc=$rc"; cat $OUT/bench.json; [ $rc -eq 0 ] || exit $rc
if [ "${PROBE:-0}" = 1 ]; then  # the per-rank share of a sharded step
  timeout -k 10 400 python -u tools/rowslice_probe.py box100k global1m > $OUT/rowslice_probe.log 2>&1
  rc=$?; echo "rowslice rc=$rc"; cut -c1-300 $OUT/rowslice_probe.log; [ $rc -eq 0 ] || exit $rc
  timeout -k 10 300 python -u tools/probe_step.py global1m 8 40 > $OUT/probe_step.log 2>&1
  rc=$?; echo "probe_step rc=$rc"; tail -1 $OUT/probe_step.log; [ $rc -eq 0 ] || exit $rc
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/probe -o run --output-format csv -- \
      python tools/probe_step.py global1m 8 30 4 > $OUT/probe_rank.log 2>&1
  rc=$?; echo "probe rc=$rc"; grep "ms per step" $OUT/probe_rank.log; [ $rc -eq 0 ] || exit $rc
  find $OUT/probe -name "*kernel_trace.csv" -size +4M -delete
fi
