# end-of-round sanity run: smoke + the full default bench + every recipe once; the bench lines go to OUT_DIR
#   tools/final_round.sh OUT_DIR
set -e
out=${1:?usage: tools/final_round.sh OUT_DIR}; mkdir -p "$out"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
python bench.py --full > "$out"/r3_final_base.json 2> "$out"/r3_final_base.err
python bench.py --full --steps 20 --warmup 5 --cpu-utts 0 --no-recall 2>/dev/null | cut -c1-160
for m in cascaded_plus hybrid_plus_large large; do python bench.py --full --model $m --steps 10 --warmup 3 --cpu-utts 0 --no-recall 2>/dev/null > "$out"/r3_final_$m.json; cut -c1-170 "$out"/r3_final_$m.json; done
python bench.py --full --trainable --steps 5 --warmup 2 --cpu-utts 0 --no-recall 2>/dev/null > "$out"/r3_final_trainable.json; cut -c1-170 "$out"/r3_final_trainable.json
python bench.py --full --unfreeze 2 --steps 10 --warmup 3 --cpu-utts 0 --no-recall 2>/dev/null > "$out"/r3_final_unfreeze2.json; cut -c1-170 "$out"/r3_final_unfreeze2.json
