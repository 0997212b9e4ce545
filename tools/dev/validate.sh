# full check of the tree on an MI355X: pytest -m gpu, smoke(), the bench line with --full
# usage: validate.sh <output directory>
set -e
OUT=${1:?usage: validate.sh <output directory>}
mkdir -p "$OUT"
timeout -k 10 1500 python -m pytest tests -m gpu -x -q > "$OUT/val_pytest.txt" 2>&1 || { tail -40 "$OUT/val_pytest.txt"; exit 1; }
tail -3 "$OUT/val_pytest.txt"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
timeout -k 10 600 python bench.py --full > "$OUT/val_bench.json" 2> "$OUT/val_bench.err"
python - "$OUT/val_bench.json" <<'P'
import json
import sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
print("bench: value", d["value"], "ms/step", d["ms_per_step"], "kernel", d["roofline"]["kernel_ms_avg"], "frac", d["roofline"]["frac"],
      "traffic", d["roofline"]["traffic"], "other", d["arithmetic"]["other_variant"]["value"], "cpu", d["cpu_baseline"]["value"], "acc", d["accuracy"]["gpu_error"])
P
