#!/bin/bash
# a host-mode kernel trace, then bench.py --full (paced density) in both modes, alternating
set -o pipefail
O=${1:-bench_out/vp8_tokens_density}
mkdir -p $O
MXDESK_VP8_TOKENS=host timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/prof_host_desktop -o k -- python bench.py --gpus 1 --codec vp8 \
  --steps 120 --warmup 10 > $O/prof_host_desktop.json 2> $O/prof_host_desktop.err || exit 1
echo "host trace done"
for i in 1 2 3; do
  for m in host gpu; do
    { TIMEFORMAT="%U user %S sys %R wall"; time env MXDESK_VP8_TOKENS=$m timeout -k 10 420 python bench.py --gpus 1 --codec vp8 --full \
      --serving-probe 0 --quality-probe 0 --steps 200 --warmup 30 > $O/full_${m}_$i.json 2> $O/full_${m}_$i.err || exit 1; } 2> $O/full_${m}_$i.time
    echo "full $m $i done"
  done
done
