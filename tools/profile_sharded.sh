#!/bin/bash
# rocprofv3 kernel stats of the column-shard path on one GPU (bench.py --sharded) -> $ESP_TOOL_OUT/kernel_stats_sharded.csv (default tool_out/)
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${ESP_TOOL_OUT:-tool_out}; mkdir -p $O   # output folder (default tool_out/)
rm -rf $O/profs
rocprofv3 --kernel-trace --stats --output-format csv -d $O/profs -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --sharded > $O/profs_bench.log 2>&1
find $O/profs -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/kernel_stats_sharded.csv
rm -rf $O/profs
grep -E '^\{' $O/profs_bench.log | tail -1 | cut -c1-260
head -14 $O/kernel_stats_sharded.csv | cut -c1-200
