#!/bin/bash
# bench.py --codec vp8 with the token partitions coded on the host and on the GPU, alternating
set -o pipefail
O=${1:-bench_out/vp8_tokens}
mkdir -p $O
for i in 1 2 3; do
  for m in host gpu; do
    { TIMEFORMAT="%U user %S sys %R wall"; time env MXDESK_VP8_TOKENS=$m MXDESK_HOST_TIMING=1 \
      timeout -k 10 150 python bench.py --gpus 1 --codec vp8 --steps 1000 --warmup 30 > $O/desktop_${m}_$i.json 2> $O/desktop_${m}_$i.err || exit 1; } 2> $O/desktop_${m}_$i.time
    echo "desktop $m $i done"
  done
done
for m in host gpu; do
  MXDESK_VP8_TOKENS=$m MXDESK_HOST_TIMING=1 timeout -k 10 150 python bench.py --gpus 1 --codec vp8 --content motion --steps 300 --warmup 30 \
    > $O/motion_${m}.json 2> $O/motion_${m}.err || exit 1
  echo "motion $m done"
done
for c in desktop motion; do
  MXDESK_VP8_TOKENS=gpu timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/prof_$c -o k -- python bench.py --gpus 1 --codec vp8 --content $c \
    --steps 120 --warmup 10 > $O/prof_$c.json 2> $O/prof_$c.err || exit 1
  echo "profile $c done"
done
