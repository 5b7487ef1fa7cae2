#!/bin/bash
# kernel statistics of the extra configs (BASELINE.json configs 3 and 4) of bench.py (run through gpurun)
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${ESP_TOOL_OUT:-tool_out}; mkdir -p $O   # output folder (default tool_out/)
rm -rf $O/profc
rocprofv3 --kernel-trace --stats --output-format csv -d $O/profc -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/profc_bench.log 2>&1
find $O/profc -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/configs_kernel_stats.csv
rm -rf $O/profc
head -24 $O/configs_kernel_stats.csv | cut -c1-200
