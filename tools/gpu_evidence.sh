#!/bin/bash
# end-of-session evidence run: parity tests, bench lines for every workload, secondary benches, PMC + kernel trace
# (logs under $OUT, default evidence_out/; the PMC passes write where tools/gpu_pmc.sh does)
export TMPDIR=/tmp
OUT=${OUT:-evidence_out}
mkdir -p $OUT
( timeout 300 python __graft_entry__.py --smoke ) > $OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/smoke.log
( timeout 1500 python -m pytest tests -m gpu -x -q -p no:cacheprovider ) > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?"
tail -2 $OUT/pytest_gpu.log
( timeout 600 python bench.py --full ) > $OUT/bench.log 2>&1; tail -1 $OUT/bench.log | cut -c1-1500
for wl in wavedec3_db2_L3_8x256x256x256_f32 wavedec2_db8_L4_64x4096x4096_f32 fswavedec2_sym16_L5_32x8192x8192_f16 wavedec_db5_L10_32x1000000_f32; do
  ( timeout 600 python bench.py --full --steps 20 --warmup 5 --workload $wl --no-cpu-baseline ) 2>/dev/null | tail -1 > $OUT/bench_$wl.log
  python -c "import json,sys; d=json.loads(open('$OUT/bench_$wl.log').read()); print('$wl', d['ms_per_step'], d['value'], d['whole_call']['frac_of_hbm_peak'], d['roofline']['frac'])"
done
( timeout 600 python tools/bench_more.py ) 2>/dev/null > $OUT/bench_more.log
( timeout 120 python tools/copy_floor.py ) 2>/dev/null > $OUT/copy_floor.log
( timeout 300 python tools/host_overhead.py ) 2>/dev/null | head -3 > $OUT/host_overhead.log
PAIR=1 RPC=0 DEPTH=0 bash tools/gpu_pmc.sh > $OUT/pmc.log 2>&1; tail -3 $OUT/pmc.log
