"""Summarise $OUT/pmc_rerank_<tag>_<pass>/ (OUT: default exp_out) (scripts/pmc_rerank.sh): SQ counters of every launch of the rerank pre-filter
kernel, the passes joined by the launch's ordinal (each pass is a run of its own with the same launches in the same order)."""
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = sys.argv[1] if len(sys.argv) > 1 else "branch"
KERNEL = sys.argv[2] if len(sys.argv) > 2 else "accurate_filtered8"
csv.field_size_limit(10**9)
launches = []  # per ordinal: counter -> value
for d in sorted(glob.glob(os.path.join(ROOT, os.environ.get("OUT", "exp_out"), f"pmc_rerank_{TAG}_[0-9]"))):
    fs = glob.glob(os.path.join(d, "*", "*counter_collection.csv"))
    if not fs:
        print(os.path.basename(d), "missing")
        continue
    fs.sort(key=os.path.getmtime)
    byd = collections.defaultdict(dict)
    for r in csv.DictReader(open(fs[-1])):
        if KERNEL in r["Kernel_Name"]:
            c = byd[int(r["Dispatch_Id"])]
            c[r["Counter_Name"]] = c.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            c["grid"], c["lds"], c["vgpr"] = int(r["Grid_Size"]), int(r.get("LDS_Block_Size", 0) or 0), int(r.get("VGPR_Count", 0) or 0)
    for i, k in enumerate(sorted(byd)):
        while len(launches) <= i:
            launches.append({})
        launches[i].update(byd[k])
print(f"{TAG}: {len(launches)} launches of {KERNEL}")


def derived(t):
    out = {}
    if "GRBM_GUI_ACTIVE" not in t or "SQ_WAVE_CYCLES" not in t:
        return out
    gui = t["GRBM_GUI_ACTIVE"] / 8  # summed over the 8 XCDs
    simd = gui * 256 * 4
    wc = 4 * t["SQ_WAVE_CYCLES"]
    out["launch_kcycles"] = gui / 1e3
    out["waves_per_simd"] = wc / simd
    out["wave_life_kcyc"] = wc / max(t.get("SQ_WAVES", 1), 1) / 1e3
    for k in ("SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_ACTIVE_INST_VMEM", "SQ_ACTIVE_INST_ANY"):  # quad-cycles, per SIMD-cycle
        if k in t:
            out[k.replace("SQ_ACTIVE_INST_", "busy_").lower()] = 4 * t[k] / simd
    for k in ("SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_SALU"):  # against one issue per 4 cycles and SIMD
        if k in t:
            out[k.replace("SQ_INSTS_", "issue_").lower()] = 4 * t[k] / simd
    for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_WAIT_INST_LDS"):  # of wave-cycles
        if k in t:
            out[k.replace("SQ_", "").lower()] = 4 * t[k] / wc
    if "SQ_LDS_BANK_CONFLICT" in t:
        out["lds_conflict_of_launch"] = t["SQ_LDS_BANK_CONFLICT"] / (gui * 256)  # cycles per CU-cycle
        if t.get("SQ_LDS_IDX_ACTIVE"):
            out["lds_conflict_of_active"] = t["SQ_LDS_BANK_CONFLICT"] / t["SQ_LDS_IDX_ACTIVE"]
    if t.get("SQ_INST_LEVEL_VMEM") and t.get("SQ_INSTS_VMEM_RD"):
        out["vmem_latency_cycles"] = t["SQ_INST_LEVEL_VMEM"] / t["SQ_INSTS_VMEM_RD"]
        out["vmem_in_flight_per_simd"] = t["SQ_INST_LEVEL_VMEM"] / simd
    return out


for i, t in enumerate(launches):
    print(f"launch {i}: grid {t.get('grid')} lds {t.get('lds')} vgpr {t.get('vgpr')}")
    print("  raw     " + "  ".join(f"{k}={v:.0f}" for k, v in sorted(t.items()) if k.startswith(("SQ_", "GRBM_"))))
    print("  derived " + "  ".join(f"{k}={v:.3f}" for k, v in derived(t).items()))
