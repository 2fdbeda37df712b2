#!/bin/bash
# quick GPU loop: parity tests, phase stamps (fused and two-launch), bench (each step time-limited;
# stop on the first failure); logs under $PFMPE_OUT (default bench_out)
cd "$(dirname "$0")/.."; out=${PFMPE_OUT:-bench_out}; mkdir -p $out
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $out/pytest_gpu.log 2>&1; rc=$?
tail -15 $out/pytest_gpu.log; [ $rc -ne 0 ] && exit $rc
PFMPE_FUSED=1 timeout -k 10 300 python scripts/diag_stamps.py ${STAMP_N:-100000} > $out/stamps.log 2>&1 || { cat $out/stamps.log; exit 1; }
cat $out/stamps.log
PFMPE_FUSED=0 timeout -k 10 300 python scripts/diag_stamps.py ${STAMP_N:-100000 1000000} > $out/stamps2.log 2>&1 || { cat $out/stamps2.log; exit 1; }
cat $out/stamps2.log
timeout -k 10 300 python bench.py --full --cpu-frames 0 > $out/bench.log 2>&1 || { tail $out/bench.log; exit 1; }
cat $out/bench.log
