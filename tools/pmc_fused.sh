# diagnostic: PMC passes over the fused kernel (separate passes; no tracing domains beside kernel-trace)
cd "$(dirname "$0")/.." && : "${PROFILE_OUT:?set PROFILE_OUT to the directory that receives the outputs}" && mkdir -p "$PROFILE_OUT"
rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS --output-format csv -d $PROFILE_OUT/pmcA -- python bench.py --steps 3 --warmup 1 --lean > $PROFILE_OUT/pmcA.log 2>&1
rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_UNALIGNED_STALL SQ_LDS_DATA_FIFO_FULL SQ_LDS_CMD_FIFO_FULL SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM --output-format csv -d $PROFILE_OUT/pmcB -- python bench.py --steps 3 --warmup 1 --lean > $PROFILE_OUT/pmcB.log 2>&1
ls $PROFILE_OUT/pmcA/*/ $PROFILE_OUT/pmcB/*/
