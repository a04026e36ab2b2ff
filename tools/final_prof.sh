set -x
export TMPDIR=/tmp
R=$PWD
O=$R/${1:?usage: bash tools/final_prof.sh OUTPUT_DIR}
mkdir -p $O/prof_final
cd /tmp
timeout 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_final -o bench -- python $R/bench.py --lean --steps 20 --warmup 5 > $O/prof_final/bench_line_under_rocprof.json 2> $O/prof_final/rocprof.log
timeout 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_f -- python $R/bench.py --lean --preroll 0 --steps 3 --warmup 1 > $O/pmc_f.log 2>&1
timeout 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_w -- python $R/bench.py --lean --preroll 0 --steps 3 --warmup 1 > $O/pmc_w.log 2>&1
cd $R
python tools/pmc_traffic.py $O/pmc_f $O/pmc_w > $O/prof_final/pmc_traffic.json
cp $O/prof_final/pmc_traffic.json profiles/r02/pmc_traffic.json
timeout 900 python bench.py --full --steps 20 --warmup 5 > $O/prof_final/bench_line_final.json 2> $O/prof_final/bench_final.err
tail -c 600 $O/prof_final/bench_line_final.json
find $O/prof_final -name "*stats*" | head
