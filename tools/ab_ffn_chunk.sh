# c4 fp32 FFN chunk size (SVOC_FFN_CHUNK): headline and the fp32 alt_precision field (--full); logs go to $OUT, default out/
OUT=${OUT:-out}
cd "$(dirname "$0")/.."; mkdir -p "$OUT"
for rep in 1 2; do
for ch in 0 16384 32768 65536; do
  SVOC_FFN_CHUNK=$ch timeout -k 10 300 python bench.py --config c4 --steps 10 --warmup 2 --full > $OUT/ffn_$ch.log 2>&1 || exit 1
  echo "chunk $ch: $(grep -o '"value": [0-9.]*' $OUT/ffn_$ch.log | head -1) $(grep -o '"alt_precision": {"encoder_dtype": "fp32", "value": [0-9.]*' $OUT/ffn_$ch.log)"
done; done
