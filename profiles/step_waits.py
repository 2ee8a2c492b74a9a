#!/usr/bin/env python3
"""Per timed step from a rocprofv3 --kernel-trace csv: end of k_insert_multi<false>, end of k_emit_meta_spec, start of the next
k_resolve_blocks4; pass 1's elapsed time; the ordinary launch gap on the resolve's queue. Usage: step_waits.py DIR K (MEASUREMENTS §0d)"""
import csv, glob, json, statistics, sys

f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
K = int(sys.argv[2])
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
for r in rows:
    r["s"], r["e"], r["n"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0]
idx = [i for i, r in enumerate(rows) if "k_resolve_blocks4" in r["n"]]
idx = idx[-(K + 1):]                       # K steps need K + 1 resolve starts; the last timed step has no successor in the trace
steps = []
gaps = []
for a, b in zip(idx[:-1], idx[1:]):
    seg = rows[a:b]
    q = rows[a].get("Queue_Id")
    t0 = rows[a]["s"]
    def last_end(name):
        v = [r["e"] for r in seg if name in r["n"]]
        return max(v) if v else None
    def first_start(name):
        v = [r["s"] for r in seg if name in r["n"]]
        return min(v) if v else None
    insF = last_end("k_insert_multi<false>")
    insT = last_end("k_insert_multi<true>")
    spec = last_end("k_emit_meta_spec")
    nxt = rows[b]["s"]
    p1a, p1b = first_start("k_emit_p1_removed"), last_end("k_spec_verify")
    raw = [r for r in seg if "k_emit_regions_raw" in r["n"]]
    comp = first_start("k_emit_p1_compact")
    st = {"wrapped": "<true>" in rows[a]["n"], "step_us": (nxt - t0) / 1e3,
          "insert_false_end": (insF - t0) / 1e3 if insF else None, "insert_true_end": (insT - t0) / 1e3 if insT else None,
          "meta_spec_end": (spec - t0) / 1e3 if spec else None,
          "next_resolve_start": (nxt - t0) / 1e3, "wait_us": (nxt - insF) / 1e3 if insF else None,
          "spec_minus_insert_us": (spec - insF) / 1e3 if spec and insF else None,
          "pass1_us": (p1b - p1a) / 1e3 if p1a and p1b else None,
          "raw_dur_us": (raw[0]["e"] - raw[0]["s"]) / 1e3 if raw else None,
          "raw_end_minus_compact_start_us": (raw[0]["e"] - comp) / 1e3 if raw and comp else None}
    for name in ("k_emit_meta_regions", "k_emit_meta_masks", "k_emit_meta_spec", "k_emit_p1_compact", "k_insert_multi<true>"):
        v = [(r["e"] - r["s"]) / 1e3 for r in seg if name in r["n"]]
        st["dur_" + name] = round(sum(v), 1) if v else None
    steps.append(st)
    main = [r for r in seg if r.get("Queue_Id") == q]
    for x, y in zip(main[:-1], main[1:]):
        gaps.append((y["s"] - x["e"]) / 1e3)

def summ(vals):
    vals = [v for v in vals if v is not None]
    if not vals:
        return None
    return {"n": len(vals), "min": round(min(vals), 1), "median": round(statistics.median(vals), 1), "max": round(max(vals), 1)}

out = {}
for tag, sel in (("before_wrap", [s for s in steps if not s["wrapped"]]), ("after_wrap", [s for s in steps if s["wrapped"]]), ("all", steps)):
    out[tag] = {k: summ([s[k] for s in sel]) for k in steps[0] if k != "wrapped"} if sel else None
pos = [g for g in gaps if g > 0.5]
out["main_queue_gaps_us"] = {"all": summ(gaps), "nonzero": summ(pos)}
out["steps"] = steps
json.dump(out, sys.stdout, indent=1)
