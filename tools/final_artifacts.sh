#!/bin/bash
# the artifacts a round ends with, run on the GPU box: OUT=<output folder> bash tools/final_artifacts.sh [bk]; everything lands in $OUT and is copied to profiles/ by hand
OUT=${OUT:?set OUT to the folder the artifacts go to}
timeout 1700 python -m pytest tests -q -m gpu 2>&1 | grep -v "^RCCL\|^HIP version\|^ROCm version\|^Hostname\|^Librccl" > $OUT/gpu_tests.log; tail -2 $OUT/gpu_tests.log
cp profiles/hbm_traffic.json $OUT/hbm_traffic.json
python bench.py --full --dump-traffic $OUT/hbm_traffic.json 2>$OUT/bench_final.err | tail -1 > $OUT/bench_final.json; wc -c $OUT/bench_final.json
if [ "${1:-}" = "bk" ]; then
  bash tools/profile_pmc.sh bk_r6final tools/bk_probe.py --default-only > $OUT/prof_bk_r6final.log 2>&1; tail -2 $OUT/prof_bk_r6final.log
  (python tools/bk_probe.py --default-only | tail -1; bash tools/probes/bk_trace.sh; python tools/bk_probe.py 18 64 --default-only | tail -1) > $OUT/bk_r6final.txt 2>&1
  exit 0
fi
bash tools/profile_bench.sh s26_r6final > $OUT/prof_s26_r6final.log 2>&1; tail -3 $OUT/prof_s26_r6final.log
bash tools/profile_pmc.sh kc22_r6final tools/kc_probe.py 22 > $OUT/prof_kc22_r6final.log 2>&1; tail -2 $OUT/prof_kc22_r6final.log
python tools/kc_probe.py 24 --ab 2>&1 | tail -4 > $OUT/kc24_r6.json
python tools/kc_probe.py 26 --ab 2>&1 | tail -4 > $OUT/kc26_r6.json
(bash tools/kc_trace.sh 26; bash tools/probes/kc_bin_traffic.sh 26; GMSX_OPT_TIMING=1 python tools/kc_probe.py 26 2>&1 | grep "kclique\]" | sort -u) > $OUT/kc26_bins_r6.txt 2>&1
(python tools/bk_probe.py --default-only | tail -1; bash tools/probes/bk_trace.sh) > $OUT/bk_r6final.txt 2>&1
GMSX_OPT_TIMING=1 python tools/probes/upload_phases.py 26 2>&1 | grep "gmsx\|rep" | grep -v "rmat\|host\]" > $OUT/upload_phases_s26.txt
