#!/bin/bash
# LDS bank-conflict cycles of the level-0 interior kernel of the exact arithmetic (bench.py --full runs it as the other
# mode), one counter run; the profiler writes under OUTPUT_DIR (relative to the repository root)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
out=${1:?usage: tools/lds_conflicts.sh OUTPUT_DIR}
rocprofv3 --kernel-trace --output-format csv --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_ACTIVE_INST_LDS -d $out -o pmc -- python bench.py --full --frames 32 --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
python - "$out" <<'PY'
import csv,glob,sys,collections
d=collections.defaultdict(list)
for f in glob.glob(sys.argv[1]+'/**/*counter_collection.csv',recursive=True):
    for r in csv.DictReader(open(f)):
        if 'level_fused<float, true, true, 32, 64' in r['Kernel_Name']:
            d[r['Counter_Name']].append(float(r['Counter_Value']))
print({k:'%.3g'%(sum(v)/len(v)) for k,v in d.items()})
PY
