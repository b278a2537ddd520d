"""profiles/k1_valu.json from one PMC pass over the K1 kernels (counters in a run of their own):
    rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVES \\
        --output-format csv -d DIR -- python3 tools/k1_partial_bench.py 32 3 0xE 0x2 0x4
    python tools/k1_valu_collect.py DIR/.../*_counter_collection.csv [slim-copy.csv [issue-cycles-<3,1> issue-cycles-<7,7>]]
The lazy route's kernel (tile_stats_bf16_rolled<3,1>) gives the headline figures, the whole-record kernel <7,7> the `whole_records` block; the
issue cost per instruction is the static mix of the listing (tools/isa_mix.py): given, or carried over from the file being replaced.
A pass over `tools/k1_partial_bench.py 32 3 0xE 0x2 0x4 --early 0.1576` also holds the early form <3,1,EARLY> at the bench's cutoff (2582 of
16 384): that launch is what the bench's timed steps issue, so it gives the headline figures then, and the plain <3,1> (cutoff 0) moves to
the `cutoff_zero` block."""
import collections
import csv
import json
import sys
from pathlib import Path

P = Path(__file__).resolve().parents[1] / "profiles"
TILES = 32 * 128 * 128


EARLY = "<3u, 1u, true, false, true>"


def per_dispatch(path, kernel_part, without=None):
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    for r in csv.DictReader(open(path)):
        if kernel_part in r["Kernel_Name"] and not (without and without in r["Kernel_Name"]):
            per[r["Counter_Name"]][int(r["Dispatch_Id"])] += float(r["Counter_Value"])
    return {c: [v for _k, v in sorted(d.items())] for c, d in per.items()}


def steady(vals):
    big = [v for v in vals if v > 0.5 * max(vals)]
    return sum(big) / len(big)


def shares(c):
    wc = steady(c["SQ_WAVE_CYCLES"])
    return {"valu_insts_per_tile": steady(c["SQ_INSTS_VALU"]) / TILES, "issuing": steady(c["SQ_ACTIVE_INST_ANY"]) / wc,
            "waiting_for_issue": steady(c["SQ_WAIT_INST_ANY"]) / wc, "waiting_for_memory": steady(c["SQ_WAIT_ANY"]) / wc}


def main():
    src = sys.argv[1]
    old = json.loads((P / "k1_valu.json").read_text())
    plain, whole = shares(per_dispatch(src, "tile_stats_bf16_rolled<3u, 1u", without=EARLY)), shares(per_dispatch(src, "tile_stats_bf16_rolled<7u, 7u"))
    early_counters = per_dispatch(src, "tile_stats_bf16_rolled" + EARLY)
    lazy = shares(early_counters) if early_counters else plain
    v = {"valu_insts_per_tile": round(lazy["valu_insts_per_tile"], 1), "avg_issue_cycles_per_inst": float(sys.argv[3]) if len(sys.argv) > 3 else old["avg_issue_cycles_per_inst"],
         "simds": old["simds"], "clock_hz": old["clock_hz"],
         "wave_cycle_shares": {k: round(x, 3) for k, x in lazy.items() if k != "valu_insts_per_tile"},
         "whole_records": dict({k: round(x, 3) for k, x in whole.items()}, avg_issue_cycles_per_inst=float(sys.argv[4]) if len(sys.argv) > 4 else old["whole_records"]["avg_issue_cycles_per_inst"]),
         **({"cutoff_zero": {k: round(x, 3) for k, x in plain.items()}} if early_counters else {}),
         "source": "rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVES on "
                   "tools/k1_partial_bench.py 32 3 0xE 0x2 0x4" + (" --early 0.1576" if early_counters else "") + (f" (profiles/{Path(sys.argv[2]).name})" if len(sys.argv) > 2 else "") +
                   (": the lazy route's K1 as the bench's timed steps launch it, tile_stats_bf16_rolled<3,1,EARLY> at cutoff 2582 of 16 384 tiles (cutoff_zero: the plain <3,1>, "
                    "which is also what roofline.kernel_alone times); issue cost carried over from the plain kernel's static mix" if early_counters else
                    ": the lazy route's K1, tile_stats_bf16_rolled<3,1>; issue cost = the kernel's static mix") + " (tools/isa_mix.py; issue rates profiles/r1_f_valu_issue_rates.txt)"}
    (P / "k1_valu.json").write_text(json.dumps(v, indent=1) + "\n")
    print(json.dumps(v, indent=1))
    if len(sys.argv) > 2:   # a slim copy of the pass for profiles/: the K1 kernels' per-dispatch sums
        agg = {}
        for r in csv.DictReader(open(src)):
            if "tile_stats_bf16_rolled" not in r["Kernel_Name"]:
                continue
            k = (r["Dispatch_Id"], r["Kernel_Name"][:80], r["Grid_Size"], r["Counter_Name"])
            agg[k] = agg.get(k, 0.0) + float(r["Counter_Value"])
        with open(sys.argv[2], "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Dispatch_Id", "Kernel_Name", "Grid_Size", "Counter_Name", "Counter_Value"])
            for (d, n, g, c), x in agg.items():
                w.writerow([d, n, g, c, f"{x:.6f}"])


if __name__ == "__main__":
    main()
