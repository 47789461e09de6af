"""Two-stream timeline of bench.py's timed loop from a rocprofv3 kernel_trace.csv.

    python scripts/stream_timeline.py kernel_trace.csv [--steps 20] [--anchor k_pnp_score_mfb<1>]

The last --steps launches of the anchor kernel (pass 1 of the bounded sequence, the only launch
that fills the chip) bound the region.  Printed: the region's span per step, the time some anchor
launch is running (the union of their intervals), the rest (the chain that the other stream's
pass 1 does not cover: "exposed"), each stream's chain time (the sum of its other launches), and the
last two steps' launches with their stream.
"""
import argparse
import csv

ap = argparse.ArgumentParser()
ap.add_argument("csv")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--anchor", default="k_pnp_score_mfb<1>")
a = ap.parse_args()

rows = list(csv.DictReader(open(a.csv)))


def stream_of(r):
    for k in ("Stream_Id", "Queue_Id"):
        if r.get(k) not in (None, ""):
            return r[k]
    return "?"


ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], stream_of(r)) for r in rows)
anch = [e for e in ev if a.anchor in e[2]]
if len(anch) < a.steps + 1:
    raise SystemExit(f"only {len(anch)} launches of {a.anchor}")
# the region: from the start of the anchor launch `steps` before the last one to the start of the last
first, last = anch[-a.steps - 1], anch[-1]
t0, t1 = first[0], last[0]
reg = [e for e in ev if e[0] >= t0 and e[0] < t1]
span = (t1 - t0) / 1e3
cover, end = 0, t0
for s, e, n, q in reg:
    if a.anchor not in n:
        continue
    s2, e2 = max(s, end), min(e, t1)
    if e2 > s2:
        cover += e2 - s2
    end = max(end, min(e, t1))
cover /= 1e3
busy_any, end = 0, t0
for s, e, n, q in reg:
    s2, e2 = max(s, end), min(e, t1)
    if e2 > s2:
        busy_any += e2 - s2
    end = max(end, min(e, t1))
busy_any /= 1e3
chain = sum(e - s for s, e, n, q in reg if a.anchor not in n) / 1e3
anchor_sum = sum(e - s for s, e, n, q in reg if a.anchor in n) / 1e3
k = a.steps
print(f"region: {k} steps, {len(reg)} launches, span {span / k:.1f} us per step")
print(f"  anchor ({a.anchor}) durations {anchor_sum / k:.1f} us per step, union {cover / k:.1f} us per step")
print(f"  other launches (the chain) {chain / k:.1f} us per step, of it exposed (no anchor running) "
      f"{(span - cover) / k:.1f} us per step = {(span - cover) / max(chain, 1e-9):.2f} of the chain")
print(f"  no kernel running at all {(span - busy_any) / k:.1f} us per step")
per = {}
for s, e, n, q in reg:
    name = n.split("(")[0].replace("void rsac::", "").replace("rsac::", "")
    d = per.setdefault(name, [0, 0.0])
    d[0] += 1
    d[1] += (e - s) / 1e3
for name, (cnt, us) in sorted(per.items(), key=lambda x: -x[1][1]):
    print(f"  {cnt / k:5.2f} x {us / cnt:7.1f} us  {name[:70]}")
tail = [e for e in ev if e[0] >= anch[-3][0] and e[0] <= last[1]]
print("last two steps (start relative to the first row, us):")
for s, e, n, q in tail:
    name = n.split("(")[0].replace("void rsac::", "").replace("rsac::", "")
    print(f"  stream {q:>4}  start {(s - tail[0][0]) / 1e3:8.1f}  dur {(e - s) / 1e3:7.1f}  {name[:60]}")
