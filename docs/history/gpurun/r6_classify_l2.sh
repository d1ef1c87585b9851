# round 6: the L2's hit rate under classify_kernel (the target's record: a random 4-byte look-up in a table of 4 bytes per read) at
# C3 (4 MB of records) and C5 (16 MB; an XCD's L2 holds 4 MB) - the verdict's item 5 asked for the rate beside the times
ROOT=$GRAFT_REPO_ROOT
OUT=$ROOT/gpurun_out/r06l2
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for wl in c3 c5; do
  rocprofv3 --kernel-trace --pmc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_EA0_RDREQ_sum --output-format csv -d $OUT/$wl -- python3 $ROOT/bench.py --workload $wl --steps 1 --warmup 0 --no-cpu-baseline --no-e2e --no-result-check > $OUT/$wl.log 2>&1 || tail -3 $OUT/$wl.log
done
cd $ROOT
python3 - <<'PY'
import csv, glob, collections, json
out = {}
for wl in ("c3", "c5"):
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    dur = collections.defaultdict(list)
    for f in glob.glob("gpurun_out/r06l2/%s/*/*counter_collection.csv" % wl):
        for row in csv.DictReader(open(f)):
            for tag in ("classify_kernel", "survivor_masks_kernel"):
                if tag in row["Kernel_Name"]:
                    per[tag][row["Counter_Name"]] += float(row["Counter_Value"])
    for f in glob.glob("gpurun_out/r06l2/%s/*/*kernel_trace.csv" % wl):
        for row in csv.DictReader(open(f)):
            for tag in ("classify_kernel", "survivor_masks_kernel"):
                if tag in row["Kernel_Name"]:
                    dur[tag].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for tag, c in per.items():
        calls = max(1, len(dur[tag]))
        hit, miss, req = c.get("TCC_HIT_sum", 0), c.get("TCC_MISS_sum", 0), c.get("TCC_REQ_sum", 0)
        out["%s %s" % (wl, tag)] = {"calls": calls, "us_per_call": round(sum(dur[tag]) / calls, 1), "TCC_REQ": req / calls, "TCC_HIT": hit / calls,
                                    "TCC_MISS": miss / calls, "hit_rate": round(hit / max(1.0, hit + miss), 4), "EA_RDREQ": c.get("TCC_EA0_RDREQ_sum", 0) / calls}
        print(wl, tag, out["%s %s" % (wl, tag)])
json.dump(out, open("gpurun_out/r06_classify_l2.json", "w"), indent=1)
PY
rm -rf $OUT
