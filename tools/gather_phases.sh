#!/bin/bash
# per-phase time of the AlphaRaw gather kernel (ADH_DEBUG_GATHER stop points) on the headline bench
for p in ${PHASES:-1 2 0}; do
  ADH_DEBUG_GATHER=$p ADH_BENCH_NO_CPU=1 python bench.py --full --steps 5 --warmup 3 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('stop', $p, 'gather %.2f ms features %.2f ms resident %.2f' % (d['roofline']['gather_kernel_ms'], d['roofline']['feature_kernel_ms'], d['resident']['ms_per_step']))"
done
