#!/bin/bash
# rocprofv3 kernel-trace summary of the bench command (same command as the
# bench line); PMC passes are separate invocations (never combined with
# tracing domains other than --kernel-trace).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
PROF=${PROF:-prof_out}  # where the rocprofv3 outputs go (scripts/summarize_profiles.py reads the same variable)
mkdir -p "$PROF"
TAG=${TAG:-r03}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PROF"/kt -o run --output-format csv -- \
    python3 bench.py --steps 10 --warmup 3 --full --no-cpu --no-ms-to-best --no-extras > "$PROF"/bench_under_rocprof.log 2>&1
rc=$?; echo "rocprof kernel-trace rc=$rc"; tail -2 "$PROF"/bench_under_rocprof.log
[ $rc -eq 0 ] || exit $rc
# C3 (BASELINE configs[2]) alone: where a 1024-problem batched call spends its time
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$PROF"/c3 -o run --output-format csv -- \
    python3 scripts/c3_prof.py > "$PROF"/c3_under_rocprof.log 2>&1
rc=$?; echo "rocprof C3 kernel-trace rc=$rc"; tail -1 "$PROF"/c3_under_rocprof.log
[ $rc -eq 0 ] || exit $rc
if [ -n "$PMC" ]; then
  timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d "$PROF"/pmc_fetch -o run --output-format csv -- \
      python3 bench.py --steps 3 --warmup 1 --full --no-cpu --no-ms-to-best --no-extras > "$PROF"/pmc_fetch.log 2>&1
  rc=$?; echo "rocprof pmc FETCH_SIZE rc=$rc"; [ $rc -eq 0 ] || exit $rc
  timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d "$PROF"/pmc_write -o run --output-format csv -- \
      python3 bench.py --steps 3 --warmup 1 --full --no-cpu --no-ms-to-best --no-extras > "$PROF"/pmc_write.log 2>&1
  rc=$?; echo "rocprof pmc WRITE_SIZE rc=$rc"; [ $rc -eq 0 ] || exit $rc
  # issue side of the same command: VALU / SALU instructions, wave-cycle split, clock
  timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY \
      SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE GRBM_COUNT \
      -d "$PROF"/pmc_valu -o run --output-format csv -- \
      python3 bench.py --steps 3 --warmup 1 --full --no-cpu --no-ms-to-best --no-extras > "$PROF"/pmc_valu.log 2>&1
  rc=$?; echo "rocprof pmc VALU rc=$rc"; [ $rc -eq 0 ] || exit $rc
  # where the waves wait: parked (s_waitcnt / barrier) vs issue stalls, and the LDS side
  timeout -s KILL 120 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_LDS \
      SQ_LDS_BANK_CONFLICT SQ_INSTS_SMEM SQ_VALU_MFMA_BUSY_CYCLES \
      -d "$PROF"/pmc_wait -o run --output-format csv -- \
      python3 bench.py --steps 3 --warmup 1 --full --no-cpu --no-ms-to-best --no-extras > "$PROF"/pmc_wait.log 2>&1
  rc=$?; echo "rocprof pmc wait rc=$rc"; [ $rc -eq 0 ] || exit $rc
  # VALU issue per quad-cycle: one or two VALU issued, MFMA co-execution
  timeout -s KILL 120 rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VALU2 SQ_VALU_MFMA_COEXEC_CYCLES \
      SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_ACTIVE_INST_SCA SQ_INSTS GRBM_GUI_ACTIVE \
      -d "$PROF"/pmc_issue -o run --output-format csv -- \
      python3 bench.py --steps 3 --warmup 1 --full --no-cpu --no-ms-to-best --no-extras > "$PROF"/pmc_issue.log 2>&1
  rc=$?; echo "rocprof pmc issue rc=$rc"; [ $rc -eq 0 ] || exit $rc
fi
find "$PROF" -name "*.csv" | head -20
