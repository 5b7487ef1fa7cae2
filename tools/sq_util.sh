cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${ESP_TOOL_OUT:-tool_out}; mkdir -p $O   # output folder (default tool_out/)
rm -rf $O/sq2
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS --kernel-trace --output-format csv -d $O/sq2 -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline ${1:---no-extra} > $O/sq2.log 2>&1
python3 tools/sq_counters.py $O/sq2 | head -${2:-4} | cut -c1-500
rm -rf $O/sq2
