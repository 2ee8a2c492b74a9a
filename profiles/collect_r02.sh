# round 2 measurements, one GPU box: bash profiles/collect_r02.sh  (then python3 profiles/assemble_r02.py here)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/r02final
rm -rf $O; mkdir -p $O
cd $R
timeout -k 10 600 python3 bench.py --full > $O/bench_full.json 2>$O/bench_full.err || exit 1
timeout -k 10 300 python3 bench.py --check --steps 2 --warmup 1 --cpu-sample 0 > $O/bench_check.json 2>$O/bench_check.err || exit 1
timeout -k 10 300 python3 bench.py --no-emit --cpu-sample 0 > $O/bench_matcher.json 2>$O/bench_matcher.err || exit 1
MBGC_BENCH_MAX_REF=4350000000 timeout -k 10 300 python3 bench.py --cpu-sample 0 > $O/bench_40bit.json 2>$O/bench_40bit.err || exit 1
SWSEM_CHAINS=1 timeout -k 10 300 python3 bench.py --cpu-sample 0 > $O/bench_one_chain_per_wave.json 2>$O/bench_one_chain.err || exit 1
timeout -k 10 300 python3 bench.py --from-host --cpu-sample 0 > $O/bench_from_host.json 2>$O/bench_from_host.err || exit 1
timeout -k 10 600 python3 profiles/cpp_host_bench.py 1000 40 5 > $O/cpp_host.json 2>$O/cpp_host.err || exit 1
timeout -k 10 600 python3 profiles/rcmatch_bench.py 256 > $O/rcmatch.json 2>$O/rcmatch.err || exit 1
timeout -k 10 300 python3 profiles/input_stage_bench.py > $O/input_stage.json 2>$O/input_stage.err || exit 1
timeout -k 10 300 python3 -m pytest tests/test_gpu_decode.py -m gpu -q -s -k full_genome > $O/decode.log 2>&1 || exit 1
export MBGC_BENCH_GEN=thread
cd /tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -- python3 $R/bench.py --cpu-sample 0 > $O/bench_rocprof.json 2>$O/kt.err || exit 1
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 400 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmc_$c -- python3 $R/bench.py --cpu-sample 0 > $O/pmc_$c.out 2>$O/pmc_$c.err || exit 1
done
timeout -k 10 400 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --kernel-trace --output-format csv -d $O/pmc_tcc -- python3 $R/bench.py --cpu-sample 0 > $O/pmc_tcc.out 2>$O/pmc_tcc.err || exit 1
timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES --kernel-trace --output-format csv -d $O/pmc_sq1 -- python3 $R/bench.py --cpu-sample 0 --steps 3 --warmup 1 --round 40 > $O/pmc_sq1.out 2>$O/pmc_sq1.err || exit 1
timeout -k 10 400 rocprofv3 --pmc SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INST_CYCLES_SALU --kernel-trace --output-format csv -d $O/pmc_sq2 -- python3 $R/bench.py --cpu-sample 0 --steps 3 --warmup 1 --round 40 > $O/pmc_sq2.out 2>$O/pmc_sq2.err || exit 1
cd $R
python3 profiles/timed_stats.py $O/kt 20 > $O/timed.json
for c in FETCH_SIZE WRITE_SIZE tcc sq1 sq2; do python3 profiles/pmc_summary.py $O/pmc_$c 20 > $O/$c.json; rm -rf $O/pmc_$c; done
cp $(find $O/kt -name "*kernel_stats.csv" | head -1) $O/kernel_stats.csv; rm -rf $O/kt
python3 profiles/kernel_stats.py $O | head -12
tail -1 $O/bench_full.json | cut -c1-400
timeout -k 10 600 python3 profiles/cpp_host_sequential.py 1000 > $O/cpp_end_to_end.json 2>$O/cpp_end_to_end.err || exit 1
MBGC_BENCH_ONE_DEVICE=1 MBGC_BENCH_BACKEND=gloo timeout -k 10 500 python3 bench.py --gpus 2 --steps 6 --warmup 3 --cpu-sample 0 > $O/bench_n2_gloo.json 2>$O/bench_n2_gloo.err || exit 1
tail -1 $O/cpp_end_to_end.json | cut -c1-300
