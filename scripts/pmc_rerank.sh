#!/bin/bash
# SQ counters of the rerank pre-filter launches (accurate_filtered8_kernel, three per step), collected in runs of their own
# (counters only with --kernel-trace), restricted to that kernel so that every other launch runs at full speed.
# Summaries under $OUT (default exp_out/; scripts/pmc_rerank_summary.py).  PMC_LIB: a library to load instead of the tree's; PMC_TAG: output suffix;
# PMC_EXTRA: further bench.py arguments, e.g. "--option scan_debug=32768" (the register kernel).
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${PMC_TAG:-branch}
[ -n "$PMC_LIB" ] && export RABITQ_HIP_SO=$PMC_LIB
ARGS="--full --steps 1 --warmup 1 --no-cpu-baseline --no-two-in-flight --no-secondary --no-batch-sweep --gt-queries 10 --small-batch 0 $PMC_EXTRA"
KERNEL=${PMC_KERNEL:-accurate_filtered8}
export OUT=${OUT:-exp_out}
mkdir -p "$OUT"
pass() {  # pass <n> <counters...>
    local n=$1; shift
    local out=$PWD/$OUT/pmc_rerank_${TAG}_$n
    rm -rf "$out"
    timeout -k 10 400 rocprofv3 --pmc "$@" --kernel-include-regex "$KERNEL" --kernel-trace --output-format csv -d "$out" -- \
        python3 bench.py $ARGS > /dev/null 2> $OUT/pmc_rerank_${TAG}_$n.log
    local rc=$?
    echo "pass $n: exit $rc"
    return $rc
}
pass 1 SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY || exit 1
pass 2 SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_VMEM || exit 1
pass 3 SQ_INST_LEVEL_VMEM SQ_INSTS_VMEM_RD SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT SQ_INSTS_SMEM || exit 1
python3 scripts/pmc_rerank_summary.py "$TAG" "$KERNEL" | tee $OUT/pmc_rerank_${TAG}_summary.txt
