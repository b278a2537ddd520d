"""GPTQ's device halves (csrc/mtq_gptq.hip) and its host factorisation, timed at DeepSeek shapes.

  gram  : mtq_gram_full over m = --tokens bf16 N(0, 1) tokens for k = 7168 and 18432; bound = m·k² bf16 MFMA flop (half of 2·m·k², the
          symmetric half) at --mfma-tflops.
  factor: gptq.factor (torch float64 Cholesky, inverse, Cholesky on the host) for k = 7168 (--factor-k).
  sweep : mtq_gptq_sweep for n × k = 7168 × 7168 and 7168 × 18432 on an upper-triangular U; bound = n·k²/2 float64 FMA at --fp64-tflops.
Wall-clock times of the best of --reps calls after a warm-up; run under `rocprofv3 --kernel-trace --stats` for kernel times.

  python tools/gptq_bench.py [--tokens 16384] [--reps 3] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import gptq as gq
from quantization_analysis_amd import hip_backend as hb


def _time(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--tokens", type=int, default=16384)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--factor-k", type=int, default=7168)
    p.add_argument("--mfma-tflops", type=float, default=2500.0, help="dense bf16 MFMA peak used for the Gram bound")
    p.add_argument("--fp64-tflops", type=float, default=78.6, help="float64 vector peak used for the sweep bound")
    p.add_argument("--json", default=None)
    args = p.parse_args()
    torch.cuda.set_device(0)
    out = []
    for k in (7168, 18432):
        x = torch.randn((args.tokens, k), device="cuda").to(torch.bfloat16)
        h = torch.zeros((k, k), dtype=torch.float64, device="cuda")
        scratch = torch.empty((max(hb.gram_full_scratch(args.tokens, k), 1),), dtype=torch.float64, device="cuda")
        t = _time(lambda: hb.gram_full(x, h, scratch), args.reps)
        bound = args.tokens * k * k / (args.mfma_tflops * 1e12)
        out.append({"what": "gram_full", "m": args.tokens, "k": k, "ms": t * 1e3, "bound_ms": bound * 1e3, "fraction": bound / t})
        print(json.dumps(out[-1]), flush=True)
        del x, h, scratch
    xk = torch.randn((4096, args.factor_k), dtype=torch.float64)
    hh = (xk.T @ xk).numpy()
    t0 = time.perf_counter()
    u = gq.factor(hh)
    out.append({"what": "factor", "k": args.factor_k, "s": time.perf_counter() - t0, "ok": not isinstance(u, str)})
    print(json.dumps(out[-1]), flush=True)
    n = 7168
    for k in (7168, 18432):
        g = torch.Generator(device="cuda").manual_seed(k)
        ud = torch.triu(torch.randn((k, k), generator=g, device="cuda", dtype=torch.float64) * (0.1 / np.sqrt(k)))
        ud.diagonal().add_(1.0)
        w = (torch.randn((n, k), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        codes = torch.full(((n + 31) // 32, (k + 31) // 32), 2, dtype=torch.int8, device="cuda")
        o = torch.empty((n, k), dtype=torch.float32, device="cuda")
        loss = torch.empty((n,), dtype=torch.float64, device="cuda")
        t = _time(lambda: hb.gptq_sweep(w, ud, codes, out=o, loss=loss), args.reps)
        bound = n * k * k / 2 * 2 / (args.fp64_tflops * 1e12)
        out.append({"what": "gptq_sweep", "n": n, "k": k, "ms": t * 1e3, "bound_ms": bound * 1e3, "fraction": bound / t})
        print(json.dumps(out[-1]), flush=True)
        del ud, w, o
    if args.json:
        Path(args.json).write_text(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
