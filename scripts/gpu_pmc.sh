#!/bin/bash
# PMC passes for the bench workload (separate runs per counter group, kernel-trace only - no sys/hip tracing).
TAG=${1:-pmc}
OUT=gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
R=$(pwd)
cd /tmp
rocprofv3 -L > $GRAFT_REPO_ROOT/$OUT/counters_list.txt 2>&1
run_pass () {
  name=$1; shift
  rm -rf /tmp/pmc_$name
  timeout 600 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d /tmp/pmc_$name -o p -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extra > $R/$OUT/run_$name.log 2>&1
  echo "rc=$?" >> $GRAFT_REPO_ROOT/$OUT/run_$name.log
  f=$(find /tmp/pmc_$name -name "*counter_collection.csv" | head -1)
  if [ -n "$f" ]; then
    # keep only our chain kernels, aggregated per (kernel, counter)
    python - "$f" > $GRAFT_REPO_ROOT/$OUT/pmc_$name.txt <<'PY'
import csv, sys, collections, re
agg = collections.defaultdict(lambda: [0.0, 0])
with open(sys.argv[1]) as fh:
    for r in csv.DictReader(fh):
        k = r.get("Kernel_Name", "")
        m = re.search(r"(chain_kernel|edge_kernel|estream_kernel|elds_kernel)<[^>]*>", k)
        if not m: continue
        key = (m.group(0), r.get("Grid_Size"), r["Counter_Name"])
        agg[key][0] += float(r["Counter_Value"]); agg[key][1] += 1
for (k, g, c), (v, n) in sorted(agg.items()):
    print(f"{k}\tgrid={g}\t{c}\tmean={v/n:.6g}\tn={n}")
PY
  fi
}
run_pass sq SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_F32 SQ_WAVES
run_pass grbm GRBM_GUI_ACTIVE GRBM_COUNT
run_pass fetch FETCH_SIZE
run_pass write WRITE_SIZE
[ "${PMC_LDS:-1}" = "1" ] && run_pass lds SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM
# summary JSON of the dominant kernel (decoder edge update = the estream_kernel / edge_kernel launch with the largest grid); bench.py reads
# the committed copy (profiles/pmc_decoder_edge.json) for roofline.traffic
python - $GRAFT_REPO_ROOT/$OUT <<'PY'
import json, sys, os, re
out = sys.argv[1]
def load(name):
    rows = {}
    p = os.path.join(out, f"pmc_{name}.txt")
    if not os.path.exists(p): return rows
    for line in open(p):
        k, g, c, v, n = line.rstrip("\n").split("\t")
        rows[(k, int(g.split("=")[1]), c)] = float(v.split("=")[1])
    return rows
r = {}
for n in ("sq", "grbm", "fetch", "write", "lds"): r.update(load(n))
# (fp32 inference runs the decoder's launch on estream_kernel - csrc/gw_edge_stream.hip - the other edge updates on edge_kernel)
edge = [(g, k) for (k, g, c) in r if k.startswith("estream_kernel")] or [(g, k) for (k, g, c) in r if k.startswith("edge_kernel")]
if edge:
    g, k = max(edge)
    get = lambda c: r.get((k, g, c))
    fetch_kib, write_kib = get("FETCH_SIZE"), get("WRITE_SIZE")
    d = {"kernel": k, "grid_threads": g,
         "FETCH_SIZE_KiB": fetch_kib, "WRITE_SIZE_KiB": write_kib,
         # MI355X_MICROARCH.md, HBM section: on gfx950 FETCH_SIZE reports half the bytes of wide coalesced reads -> x2
         "hbm_read_bytes": None if fetch_kib is None else 2.0 * fetch_kib * 1024.0,
         "hbm_write_bytes": None if write_kib is None else write_kib * 1024.0,
         "SQ_VALU_MFMA_BUSY_CYCLES": get("SQ_VALU_MFMA_BUSY_CYCLES"), "SQ_INSTS_VALU_MFMA_F32": get("SQ_INSTS_VALU_MFMA_F32"),
         "GRBM_GUI_ACTIVE": get("GRBM_GUI_ACTIVE"), "SQ_WAVE_CYCLES": get("SQ_WAVE_CYCLES"), "SQ_WAIT_ANY": get("SQ_WAIT_ANY"),
         "SQ_WAIT_INST_ANY": get("SQ_WAIT_INST_ANY"), "SQ_LDS_BANK_CONFLICT": get("SQ_LDS_BANK_CONFLICT")}
    if d["SQ_VALU_MFMA_BUSY_CYCLES"] and d["GRBM_GUI_ACTIVE"]:
        # busy cycles are summed over the 1024 SIMDs, GRBM_GUI_ACTIVE over the 8 XCDs
        d["mfma_busy_frac"] = d["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0 / (d["GRBM_GUI_ACTIVE"] / 8.0)
    json.dump(d, open(os.path.join(out, "pmc_decoder_edge.json"), "w"), indent=1)
    print(json.dumps(d))
PY
ls -la $GRAFT_REPO_ROOT/$OUT
tail -n 60 $GRAFT_REPO_ROOT/$OUT/pmc_sq.txt
