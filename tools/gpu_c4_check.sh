#!/bin/bash
# c4 encoder: GPU kernel tests (bf16 + fp32), then the c4 bench (bf16 headline + fp32 alt_precision field: --full)
# (logs go to $OUT, default out/)
OUT=${OUT:-out}
cd "$(dirname "$0")/.."; mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests/test_encoder_ops_gpu.py -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider > $OUT/pt_enc.log 2>&1; rc=$?; tail -15 $OUT/pt_enc.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 500 python bench.py --config c4 --steps 10 --warmup 2 --full > $OUT/b_c4.log 2>&1 || { tail -5 $OUT/b_c4.log; exit 1; }
grep '^{' $OUT/b_c4.log
