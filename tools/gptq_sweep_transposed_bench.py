"""mtq_gptq_sweep_transposed (csrc/mtq_gptq_transpose.hip) against mtq_gptq_sweep (csrc/mtq_gptq.hip): bfp4 codes, bf16 W, an
upper-triangular U, at n = k = 4096 and 7168.  After a warm-up of both, --reps timed regions per kernel, alternating between the two,
each between two device events; the medians and the spread (min, max) are printed, one JSON line per shape.  Ŵ of the two layouts
differs by design (another grouping); each kernel's output is checked to be deterministic across the timed calls.

  python tools/gptq_sweep_transposed_bench.py [--reps 7] [--sizes 4096 7168] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import hip_backend as hb


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 7168])
    p.add_argument("--json", default=None)
    args = p.parse_args()
    torch.cuda.set_device(0)
    out = []
    for k in args.sizes:
        n = k
        g = torch.Generator(device="cuda").manual_seed(k)
        ud = torch.triu(torch.randn((k, k), generator=g, device="cuda", dtype=torch.float64) * (0.1 / np.sqrt(k)))
        ud.diagonal().add_(1.0)
        w = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        codes = torch.full(((n + 31) // 32, (k + 31) // 32), 2, dtype=torch.int8, device="cuda")     # square: the same shape in both grids
        routes = {"rows": hb.gptq_sweep, "transpose": hb.gptq_sweep_transposed}
        bufs = {name: (torch.empty((n, k), dtype=torch.float32, device="cuda"), torch.empty((n,), dtype=torch.float64, device="cuda"))
                for name in routes}
        first = {}
        for name, fn in routes.items():                                                              # warm-up, and the outputs to compare
            fn(w, ud, codes, out=bufs[name][0], loss=bufs[name][1])
            torch.cuda.synchronize()
            first[name] = (bufs[name][0].clone(), bufs[name][1].clone())
        ms = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(w, ud, codes, out=bufs[name][0], loss=bufs[name][1])
                b.record()
                torch.cuda.synchronize()
                ms[name].append(a.elapsed_time(b))
        row = {"n": n, "k": k, "reps": args.reps}
        for name in routes:
            same = bool(torch.equal(first[name][0], bufs[name][0]) and torch.equal(first[name][1], bufs[name][1]))
            row[name] = {"median_ms": statistics.median(ms[name]), "min_ms": min(ms[name]), "max_ms": max(ms[name]), "deterministic": same,
                         "loss_sum": float(bufs[name][1].sum())}
        row["transpose_over_rows"] = row["transpose"]["median_ms"] / row["rows"]["median_ms"]
        out.append(row)
        print(json.dumps(row), flush=True)
        del ud, w, bufs, first
    if args.json:
        Path(args.json).write_text(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
