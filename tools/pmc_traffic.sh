# diagnostic: HBM traffic of the fused kernel (FETCH_SIZE and WRITE_SIZE in separate passes)
cd "$(dirname "$0")/.." && : "${PROFILE_OUT:?set PROFILE_OUT to the directory that receives the outputs}" && mkdir -p "$PROFILE_OUT"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $PROFILE_OUT/pmcF -- python bench.py --steps 3 --warmup 1 --lean > $PROFILE_OUT/pmcF.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $PROFILE_OUT/pmcW -- python bench.py --steps 3 --warmup 1 --lean > $PROFILE_OUT/pmcW.log 2>&1
ls $PROFILE_OUT/pmcF/*/ $PROFILE_OUT/pmcW/*/
