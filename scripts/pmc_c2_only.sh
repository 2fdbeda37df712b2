#!/bin/bash
# Round-2 measurement pass: the default bench line (C2 + cpu_baseline + worst case + multi-stream sweep),
# C3 / C4 / C5 lines, rocprofv3 kernel stats of C2, C4, C5 and a 16-stream C2 batch, the C4, C5 and 16-stream PMC
# passes, and the initialisation bench.  Every GPU step has its own time limit; a failure stops the script.
# Output under $PFMPE_OUT (default bench_out).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
out=${PFMPE_OUT:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
t=${TAG:-r02}
run() {  # run <name> <limit-s> <cmd...>
  local name=$1 lim=$2; shift 2
  echo "== $name $(date +%T)"
  timeout -k 10 "$lim" "$@" > "$out/${t}_$name.log" 2>&1
  local rc=$?
  tail -c 300 "$out/${t}_$name.log"; echo
  if [ $rc -ne 0 ]; then echo "STOP after $name rc=$rc"; exit $rc; fi
}
pmc() {  # pmc <name> <bench args> -- counters per pass as separate runs
  local name=$1 args=$2; local i=0
  for set in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_WAVE_CYCLES" \
             "SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INST_CYCLES_VMEM_RD GRBM_GUI_ACTIVE" \
             "SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_INT64 SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS" \
             "FETCH_SIZE" "WRITE_SIZE"; do
    i=$((i+1))
    run pmc_${name}_p$i 120 rocprofv3 --pmc $set --output-format csv -d $out/${t}_pmc_$name/p$i -o run -- python3 bench.py --full --cpu-frames 0 --no-timing --worst-frames 0 $args
  done
  python3 scripts/pmc_summary.py $out/${t}_pmc_$name --json $out/${t}_pmc_$name.json > $out/${t}_pmc_$name.txt 2>&1
}
pmc c2 "--steps 50 --warmup 5 --multi-steps 5"
echo "== done $(date +%T)"
