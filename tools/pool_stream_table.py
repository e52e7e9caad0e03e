"""Per-geometry table of the pooling launches of tools/pool_stream_bench.py.

    python tools/pool_stream_table.py <tag> <plan.json> <csv> [<csv> ...]

Each csv is a rocprofv3 kernel trace (`*kernel_trace.csv`: one run = one column of per-launch medians, so three
traces of one build give its run-to-run spread) or a counter pass (`*counter_collection.csv`: FETCH_SIZE doubled as
MI355X_MICROARCH.md prescribes for gfx950, WRITE_SIZE, and whatever SQ_* counters were collected, per launch).
Dispatches are matched to the plan by launch order among the kernels whose name contains `pool`.
Prints one line per geometry: median microseconds per launch of each trace, the fraction of 8 TB/s that the
algorithmic bytes reach at the median of those, and the counters.
"""
import csv
import json
import statistics
import sys

tag, plan_path, paths = sys.argv[1], sys.argv[2], sys.argv[3:]
plan = json.load(open(plan_path))
need = sum(e["kernels"] * e["reps"] for e in plan)


def pool_rows(rows):
    return [r for r in rows if "pool" in r["Kernel_Name"] and "avgpool" not in r["Kernel_Name"]]


times, counters = [], {}
for p in paths:
    rows = list(csv.DictReader(open(p)))
    if "Counter_Name" in rows[0]:
        per = {}
        for r in rows:
            if "pool" in r["Kernel_Name"] and "avgpool" not in r["Kernel_Name"]:
                d = per.setdefault(int(r["Dispatch_Id"]), {})
                d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
        ids = sorted(per)
        if len(ids) != need:
            raise SystemExit("%s: %d pooling dispatches, the plan has %d" % (p, len(ids), need))
        i = 0
        for e in plan:
            n = e["kernels"] * e["reps"]
            for c in set().union(*(per[j] for j in ids[i:i + n])):
                counters.setdefault(e["label"], {})[c] = sum(per[j].get(c, 0.0) for j in ids[i:i + n]) / e["reps"]
            i += n
    else:
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        rows = pool_rows(rows)
        if len(rows) != need:
            raise SystemExit("%s: %d pooling dispatches, the plan has %d" % (p, len(rows), need))
        col, i = {}, 0
        for e in plan:
            per_call = []
            for r in range(e["reps"]):
                part = rows[i:i + e["kernels"]]
                per_call.append(sum(int(q["End_Timestamp"]) - int(q["Start_Timestamp"]) for q in part) / 1e3)
                i += e["kernels"]
            col[e["label"]] = statistics.median(per_call)
        times.append(col)

print("# %s: microseconds per launch (median of the repetitions), one column per traced run; fraction of 8 TB/s from "
      "the algorithmic bytes at the median column" % tag)
cn = sorted({c for v in counters.values() for c in v})
print("%-44s %9s  %-27s %6s %s" % ("launch", "alg MB", "us per run", "of 8T", " ".join(cn)))
tot = [0.0] * len(times)
for e in plan:
    t = [c[e["label"]] for c in times]
    for i, v in enumerate(t):
        tot[i] += v
    med = statistics.median(t) if t else 0.0
    frac = e["bytes"] / (med * 1e-6) / 8e12 if med else 0.0
    cs = counters.get(e["label"], {})
    cv = []
    for c in cn:
        v = cs.get(c, 0.0)
        if c == "FETCH_SIZE":
            cv.append("fetch %.1f MB" % (v * 2e3 / 1e6))
        elif c == "WRITE_SIZE":
            cv.append("write %.1f MB" % (v * 1e3 / 1e6))
        else:
            cv.append("%s %.4g" % (c, v))
    print("%-44s %9.1f  %-27s %6.2f %s" % (e["label"], e["bytes"] / 1e6, " ".join("%8.1f" % v for v in t), frac,
                                          "; ".join(cv)))
print("%-44s %9s  %-27s" % ("total", "", " ".join("%8.1f" % v for v in tot)))
