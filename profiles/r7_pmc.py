"""Reduces the rocprofv3 output of a parent / new pair of runs (kernel trace with --stats, two SQ counter passes, each a run of its own) to the
figures profiles/r7_pass_slices.md and profiles/pmc_cornell.json quote: per tag, the megakernel's time, its SQ counters summed over the
dispatches of the run, VALU wave-instructions per path and lane utilisation. Usage: r7_pmc.py DIR [paths per dispatch], DIR holding
<tag>_stats, <tag>_sq1, <tag>_sq2 for tag in parent, new."""
import csv
import glob
import json
import os
import sys


def rows(d, suffix):
    for f in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        with open(f, newline="") as fh:
            yield from csv.DictReader(fh)


def main():
    root = sys.argv[1]
    paths = float(sys.argv[2]) if len(sys.argv) > 2 else 1024.0 * 1024.0 * 1024.0
    out = {}
    for tag in ("parent", "new"):
        r = {}
        ms = [(float(x["End_Timestamp"]) - float(x["Start_Timestamp"])) / 1e6 for x in rows(os.path.join(root, tag + "_stats"), "kernel_trace.csv")
              if "pathTraceKernel" in x.get("Kernel_Name", "")]
        r["kernel"] = sorted({x["Kernel_Name"] for x in rows(os.path.join(root, tag + "_stats"), "kernel_trace.csv") if "pathTraceKernel" in x.get("Kernel_Name", "")})
        r["kernel_ms_per_dispatch"] = [round(m, 3) for m in ms]
        ctr, disp = {}, set()
        for p in ("_sq1", "_sq2"):
            for x in rows(os.path.join(root, tag + p), "counter_collection.csv"):
                if "pathTraceKernel" not in x.get("Kernel_Name", ""):
                    continue
                disp.add((p, x.get("Dispatch_Id")))
                ctr[x["Counter_Name"]] = ctr.get(x["Counter_Name"], 0.0) + float(x["Counter_Value"])
        n = max(1, len({d for q, d in disp if q == "_sq1"}))
        r["dispatches_under_pmc"] = n
        r["counters"] = ctr
        if "SQ_INSTS_VALU" in ctr:
            r["valu_insts_per_path"] = ctr["SQ_INSTS_VALU"] / (paths * n)
        if "SQ_THREAD_CYCLES_VALU" in ctr and "SQ_ACTIVE_INST_VALU" in ctr:
            r["lane_utilisation"] = round(ctr["SQ_THREAD_CYCLES_VALU"] / (64.0 * ctr["SQ_ACTIVE_INST_VALU"]), 4)
        if "SQ_WAIT_ANY" in ctr and "SQ_WAVE_CYCLES" in ctr:
            r["wait_any_frac"] = round(ctr["SQ_WAIT_ANY"] / ctr["SQ_WAVE_CYCLES"], 4)
        out[tag] = r
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
