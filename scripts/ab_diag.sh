#!/bin/bash
# A/B of diagnostic switches (bench --diag) on the in-tree library, alternating; each run time-limited;
# logs under $PFMPE_OUT (default bench_out)
cd "$(dirname "$0")/.."; out=${PFMPE_OUT:-bench_out}; mkdir -p $out
for r in 1 2 3; do
  for d in ${AB_DIAGS:-0 64 128}; do
    timeout -k 10 300 python bench.py --full --cpu-frames 0 --steps 400 --warmup 40 --diag $d > $out/abd_$d.log 2>&1 || { tail $out/abd_$d.log; exit 1; }
    python3 -c "import json; d=json.load(open('$out/abd_$d.log')); print('diag $d', round(d['ms_per_step']*1e3,2), 'us/frame', d['roofline']['per_kernel_avg_us'])"
  done
done
