#!/bin/bash
# A/B of library variants over quick benches: tools/ab.sh base <variant> ...
# (base = libastyle.so, else libastyle_<variant>.so built by ASTYLE_VARIANT=... _build.py, or any
# library put there under that name, e.g. the parent commit's); a name may repeat (alternating
# runs: tools/ab.sh parent base parent base parent base).  $AB_ARGS: more bench.py arguments
# (e.g. "--precision fp32 --clips 1 --steps 50"); logs go to $BENCH_OUT (default bench_out/)
set -o pipefail
O=${BENCH_OUT:-bench_out}
mkdir -p $O
N=0
for V in "$@"; do
  N=$((N + 1))
  if [ $V = base ]; then L=audio_style_transfer_amd/libastyle.so; else L=audio_style_transfer_amd/libastyle_$V.so; fi
  ASTYLE_LIB=$L timeout -k 10 200 python bench.py --full --cpu-baseline-seconds 0 --side-steps 0 $AB_ARGS > $O/ab_${N}_$V.log 2>&1 || { echo "$V failed"; tail $O/ab_${N}_$V.log; exit 1; }
  python -c "import json; d=json.loads(open('$O/ab_${N}_$V.log').read().strip().splitlines()[-1]); r=d['roofline']; k=d['kernels_ms_per_step']; print('$V', round(d['value'],3), 'ms/step', round(d['config']['global_batch_clips'] / 256.0 / d['value'] * 1e3, 3), 'fwd', round(r['fwd']['launch_ms'],4), 'bwd', round(r['bwd']['launch_ms'],4), 'gram', round(k['gram_fwd'],3), round(k['gram_bwd'],3), 'grad', d['grad_rel_l2'])"
done
