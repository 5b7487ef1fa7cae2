cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${ESP_TOOL_OUT:-tool_out}; mkdir -p $O   # output folder (default tool_out/)
for st in 1 2 3 0; do
  rm -rf $O/sqs
  ESP_LOCAL_STOP=$st rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --kernel-trace --output-format csv -d $O/sqs -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/sqs.log 2>&1
  echo "stop=$st"; python tools/sq_counters.py $O/sqs | grep local_k | cut -c1-300
done
rm -rf $O/sqs
