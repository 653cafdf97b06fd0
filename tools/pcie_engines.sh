# The host-buffer (PCIe-inclusive) leg of bench.py with 1 / 2 / 4 engines on as many host
# threads, pageable and page-locked caller buffers -> $OUT/pcie_ab.txt
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/build/bench}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
: > $OUT/pcie_ab.txt
for E in 1 2 4; do
  timeout -k 10 400 python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-isolated --pcie-engines $E > $OUT/pcie_$E.json 2>$OUT/pcie_$E.err || { tail -3 $OUT/pcie_$E.err; exit 1; }
  python3 -c "
import json; d=json.loads(open('$OUT/pcie_$E.json').read().strip().splitlines()[-1]); p=d['pcie_inclusive']; q=p['pinned']
print('pcie engines $E pageable', round(p['value']), 'ms %.2f' % p['ms_per_step'], '| pinned', round(q['value']), 'ms %.2f' % q['ms_per_step'], q['ms_per_step_all'])" | tee -a $OUT/pcie_ab.txt
done
