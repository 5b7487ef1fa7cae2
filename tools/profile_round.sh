cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${ESP_TOOL_OUT:-tool_out}; mkdir -p $O   # output folder (default tool_out/)
rm -rf $O/prof $O/pmc_f $O/pmc_w
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-extra > $O/prof_bench.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_f -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extra > $O/pmc_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_w -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extra > $O/pmc_w.log 2>&1
python3 tools/pmc_traffic.py $O/pmc_f $O/pmc_w $O/pmc_traffic.json ${1:-r2} > /dev/null
find $O/prof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/kernel_stats.csv
rm -rf $O/prof $O/pmc_f $O/pmc_w
tail -1 $O/prof_bench.log | cut -c1-300
head -12 $O/kernel_stats.csv
