#!/bin/bash
# usage: pmc_kernel.sh "<COUNTER ...>" <kernel-name-substring> [OUTDIR]   (on an MI355X; trace under OUTDIR, default $TMPDIR/bzh_pmc_k)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${3:-$TMPDIR/bzh_pmc_k}
rm -rf "$OUT/trace" && mkdir -p "$OUT"
rocprofv3 --pmc $1 --kernel-trace --output-format csv -d "$OUT/trace" -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu > "$OUT/pmc_k.log" 2>&1
python3 - "$2" "$OUT/trace" <<'PY'
import csv, glob, collections, sys, os
f = max(glob.glob(f'{sys.argv[2]}/*/*counter_collection.csv'), key=os.path.getsize)
agg = collections.defaultdict(lambda: collections.defaultdict(float)); n = collections.Counter()
for r in csv.DictReader(open(f)):
    k = r['Kernel_Name'].split('(')[0].replace('void ', '')
    if sys.argv[1] in k:
        agg[k][r['Counter_Name']] += float(r['Counter_Value']); n[(k, r['Counter_Name'])] += 1
for k, d in agg.items():
    print(k, {c: (round(v), n[(k, c)]) for c, v in d.items()})
PY
