"""Per-kernel durations of the y-form sweep's passes from a rocprofv3 kernel
trace of the bench command: mean / median microseconds and launch count of
the start pass, the first step (k_spmm_lanczos_first, compact sweeps), the
second step (k_spmm_lanczos with the int16 Yold flag, bit 7), the ordinary
pass and the last pass.
Usage: python tools/first_step_trace.py KERNEL_TRACE_CSV  (prints JSON)"""
import collections
import csv
import json
import re
import sys


def main(path):
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        m = re.search(r"kt::(k_\w+)<([^>]*)>", r["Kernel_Name"])
        if not m or not m.group(1).startswith(("k_spmm_lanczos", "k_spmm_quadform", "k_ycoef")):
            continue
        agg[f"{m.group(1)}<{m.group(2)}>"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    out = {}
    for k, v in sorted(agg.items()):
        v.sort()
        out[k] = {"launches": len(v), "mean_us": round(sum(v) / len(v), 2), "median_us": round(v[len(v) // 2], 2)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
