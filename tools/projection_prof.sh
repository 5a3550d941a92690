#!/usr/bin/env bash
# counters of the projection kernels beside the unshaded march's, run ON the GPU box: bash tools/projection_prof.sh <outdir> [states...]
# One rocprofv3 --pmc run per counter set and state, without any tracing; the program is tools/projection_bench.py --profile-state (1024^3 f32, 1920 x 1080).
# (Each set fits one pass of the hardware's counters; a set that does not makes the profiler give up before the program runs.)
# Writes <outdir>/pmc_summary.txt: per state, kernel and counter the mean per dispatch over the frames.
set -uo pipefail
out=$1; shift
states=${*:-baseline maximum mean}
mkdir -p "$out"
: > "$out/pmc_summary.txt"
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_INSTS_LDS" \
           "TA_BUSY_sum TA_TA_BUSY_sum TCP_PENDING_STALL_CYCLES_sum TD_TD_BUSY_sum" \
           "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCC_HIT_sum TCC_MISS_sum"; do
  i=$((i + 1))
  for state in $states; do
    d="$out/raw_${state}_$i"
    timeout -k 10 240 rocprofv3 --pmc $set --output-format csv -d "$d" -- python3 tools/projection_bench.py c3 --profile-state "$state" --settle 3 --frames 8 > "$out/run_${state}_$i.log" 2>&1
    rc=$?
    case $rc in 124|137|134|139) echo "state $state set $i ended with $rc: stopping" | tee -a "$out/error"; exit $rc;; esac
    [ $rc -ne 0 ] && echo "pmc set failed ($rc): $state: $set" >> "$out/error"
    python3 - "$d" "$state" >> "$out/pmc_summary.txt" <<'PY'
import collections, csv, glob, sys
agg = collections.defaultdict(lambda: [0, 0.0])
for f in sorted(glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0]
        if "project_kernel" in k or "raymarch_kernel" in k:
            a = agg[(k[:60], r["Counter_Name"])]
            a[0] += 1; a[1] += float(r["Counter_Value"])
for (k, c), (n, v) in sorted(agg.items()):
    print(f"{sys.argv[2]} {k} {c} dispatches={n} mean={v / n:.6g}")
PY
    rm -rf "$d"
  done
done
