"""profiles/pmc_score_valu.json and pmc_score_kernel.json for the bounded scoring sequence
(DESIGN.md §16): bench.py --full divides their per-launch figures by score_ms, which now spans
the step's five scoring launches, so each figure is the sum over those launches of the kernel's
median per-launch counter.

    python scripts/bound_pmc.py DIR [OUT]

DIR/pmc_valu, DIR/pmc_fetch, DIR/pmc_write: one rocprofv3 --pmc run each (SQ_INSTS_VALU
SQ_INSTS_SALU / FETCH_SIZE / WRITE_SIZE, the program after --, no tracing beside it) of
python bench.py --steps 3 --warmup 1 --full --no-cpu --no-ms-to-best --no-extras.
OUT: where the two files go (default profiles/).
"""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the launches between the scoring events of rsac_pnp_evaluate_range (launch_pnp_score_bounded): the
# hinted sequence that every call after a context's first one on a problem takes (pass 0 inside pass
# 1's launch, the plan inside select), or the five-launch sequence of a build without it
# (-DRSAC_BOUND_HINT=0).  A hinted run also holds each context's first, unhinted call: the medians
# are the hinted launches', and the five-launch kernels' few rows are reported, not summed.
HINTED = ["k_pnp_score_mfb<1>", "k_pnp_bound_select_plan", "k_pnp_score_mfb<2>"]
UNHINTED = ["k_pnp_score_mf<4>", "k_pnp_bound_plan", "k_pnp_score_mfb<1>", "k_pnp_bound_select", "k_pnp_score_mfb<2>"]


def step_sum(d, name):
    """(sum over the step's kernels of the median per-launch value of counter `name`, {kernel: median},
    launches, the sequence found); the sequence is chosen from the launches present, and anything
    else than one of the two sequences, whole, ends the run"""
    path = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0]
    per = {}
    for row in csv.DictReader(open(path)):
        if row["Counter_Name"] == name:
            k = next((s for s in set(HINTED + UNHINTED) if "rsac::" + s + "(" in row["Kernel_Name"]), None)
            if k:
                per[(k, row["Dispatch_Id"])] = per.get((k, row["Dispatch_Id"]), 0.0) + float(row["Counter_Value"])
    by = {}
    for (k, _), v in per.items():
        by.setdefault(k, []).append(v)
    hinted = "k_pnp_bound_select_plan" in by
    step = HINTED if hinted else UNHINTED
    missing = [s for s in step if s not in by]
    if missing:
        raise SystemExit(f"{path}: no {name} rows for {missing} of the {'hinted' if hinted else 'five-launch'} sequence")
    n = min(len(by[k]) for k in step)
    if hinted:
        # the unhinted first calls must be few beside the hinted ones, or the medians mix the two
        first = max((len(by[k]) for k in UNHINTED if k not in HINTED and k in by), default=0)
        if 2 * first >= n:
            raise SystemExit(f"{path}: {first} unhinted first calls beside {n} hinted ones: run more steps")
    med = {k: statistics.median(by[k]) for k in step}
    return sum(med.values()), med, n, "hinted" if hinted else "five-launch"


def main():
    d = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
    points, hyps = 10_000, 100_000
    valu, valu_by, n, seq = step_sum(os.path.join(d, "pmc_valu"), "SQ_INSTS_VALU")
    salu, _, _, _ = step_sum(os.path.join(d, "pmc_valu"), "SQ_INSTS_SALU")
    json.dump({"kernel": "k_pnp_score", "points": points, "hyps": hyps, "launches": n,
               "sequence": seq, "valu_instr_per_launch": valu, "salu_instr_per_launch": salu, "valu_by_kernel": valu_by,
               "note": "the hinted bounded scoring sequence: sum over the step's scoring launches (pass 1 with "
                       "pass 0 inside, select with the plan, pass 2) of each kernel's median per-launch count; bench.py divides it by score_ms, "
                       "which spans the same launches"},
              open(os.path.join(out, "pmc_score_valu.json"), "w"), indent=1)
    fk, fk_by, n, _ = step_sum(os.path.join(d, "pmc_fetch"), "FETCH_SIZE")
    wk, wk_by, _, _ = step_sum(os.path.join(d, "pmc_write"), "WRITE_SIZE")
    json.dump({"kernel": "k_pnp_score", "points": points, "hyps": hyps, "fetch_size_kib": fk, "write_size_kib": wk,
               "hbm_bytes_per_launch": (2.0 * fk + wk) * 1024.0, "algorithmic_bytes_per_launch": points * 20 * hyps,
               "launches": n, "fetch_kib_by_kernel": fk_by, "write_kib_by_kernel": wk_by,
               "note": "the bounded scoring sequence: sums over the step's scoring launches; FETCH_SIZE doubled per "
                       "MI355X_MICROARCH.md (HBM); counters in KiB"},
              open(os.path.join(out, "pmc_score_kernel.json"), "w"), indent=1)
    print(seq, "valu", valu, valu_by)
    print("fetch KiB", fk, "write KiB", wk)


if __name__ == "__main__":
    main()
