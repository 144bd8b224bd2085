# collects the judged evidence for profiles/: bench line, rocprof kernel stats (>= 50 timed steps, so that the AVERAGE -- not
# the minimum -- supports the quoted fraction), PMC passes (each in its own run), and the same for config 3's shape
cd "$(dirname "$0")/.." && : "${PROFILE_OUT:?set PROFILE_OUT to the directory that receives the outputs}" && mkdir -p "$PROFILE_OUT"
python bench.py --full --steps 20 --warmup 5 > $PROFILE_OUT/bench_final.json 2> $PROFILE_OUT/bench_final.err
tail -1 $PROFILE_OUT/bench_final.json | cut -c1-300
rocprofv3 --kernel-trace --stats --output-format csv -d $PROFILE_OUT/profS -- python bench.py --steps 60 --warmup 10 --lean > $PROFILE_OUT/profS.log 2>&1
bash tools/pmc_fused.sh > $PROFILE_OUT/pmc_run.log 2>&1
bash tools/pmc_traffic.sh > $PROFILE_OUT/pmc_traffic.log 2>&1
# config 3's shape (one 1.25M-row shard, B = 1024, k = 100): kernel stats + the FETCH_SIZE / WRITE_SIZE passes of the wide kernel
python bench.py --full --config c3 --steps 20 --warmup 5 --no-cpu > $PROFILE_OUT/bench_c3.json 2> $PROFILE_OUT/bench_c3.err
rocprofv3 --kernel-trace --stats --output-format csv -d $PROFILE_OUT/profS3 -- python bench.py --config c3 --steps 30 --warmup 5 --lean > $PROFILE_OUT/profS3.log 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $PROFILE_OUT/pmcF3 -- python bench.py --config c3 --steps 3 --warmup 1 --lean > $PROFILE_OUT/pmcF3.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $PROFILE_OUT/pmcW3 -- python bench.py --config c3 --steps 3 --warmup 1 --lean > $PROFILE_OUT/pmcW3.log 2>&1
python bench.py --full --config c1 --steps 200 --warmup 20 > $PROFILE_OUT/bench_c1.json 2> $PROFILE_OUT/bench_c1.err
python bench.py --full --config c4 --steps 20 --warmup 5 --no-cpu > $PROFILE_OUT/bench_c4.json 2> $PROFILE_OUT/bench_c4.err
ls $PROFILE_OUT/profS/*/ $PROFILE_OUT/profS3/*/ $PROFILE_OUT/pmcF3/*/ | head -30
