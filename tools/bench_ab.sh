#!/bin/bash
# A/B of the product build against a variant build (cvpr2025-decafnet_amd/build/variants/<name>) on the default bench workload, alternating
# inside ONE GPU call (boxes differ by several per cent between calls).  Prints clips/s, the event time per forward and the stage times
# that are named on the command line.
#   tools/bench_ab.sh <variant> [rounds] [stage substring ...]
R=${GRAFT_REPO_ROOT:-/root/repo}
V=${1:-base}; N=${2:-2}; shift; shift
cd "$R" || exit 1
OUT=$(mktemp -d)
LIB="$R/cvpr2025-decafnet_amd/build/variants/$V/libdecafnet_hip.so"
test -f "$LIB" || { echo "no variant $V"; exit 1; }
show() {
python3 - "$1" "${@:2}" <<'P'
import json, sys
d = None
for line in open(sys.argv[1]):
    line = line.strip()
    if line.startswith('{'):
        d = json.loads(line)
if d is None:
    print('no JSON line'); sys.exit(0)
st = d.get('stages', {})
pick = {k: round(v['ms_per_step'], 4) for k, v in st.items() if any(s in k for s in sys.argv[2:])}
print(f"{d['value'] / 1e6:7.3f} M clips/s  event ms {d.get('event_ms_per_step', 0):.3f}  frac {d['roofline']['frac']:.4f}  {pick}")
P
}
for i in $(seq "$N"); do
  python3 bench.py --full --min-timed-s 2 --no-post --no-cpu-baseline > "$OUT/ab_prod.json" 2> "$OUT/ab_prod.err"; echo -n "product  "; show "$OUT/ab_prod.json" "$@"
  DCF_LIB_PATH=$LIB python3 bench.py --full --min-timed-s 2 --no-post --no-cpu-baseline > "$OUT/ab_var.json" 2> "$OUT/ab_var.err"; echo -n "$V  "; show "$OUT/ab_var.json" "$@"
done
