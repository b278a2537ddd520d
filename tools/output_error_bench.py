"""Layer-output error: the fused kernel (csrc/mtq_output_error.hip) against the unfused torch route on the same GPU.

Shapes: every 2-D weight of the synthetic:deepseek-r1-layer0 preset plus the three layer-0 MLP weights (gate / up 18432×7168,
down 7168×18432; float32 fp8-block-like values as the loader returns DeepSeek weights), M = 12 800 synthetic N(0, 1) bf16 tokens,
candidates bf16, bfp8, bfp4, bfp2 and the reference.
  fused   : one mtq_output_error launch (+ its reduction) over all of X.
  unfused : per format K2 → bf16 Ŵ → torch.matmul (bf16 out) → torch float64 reductions of the seven sums; the reference
            R = X·bf16(W)ᵀ by one torch.matmul.  (Cheaper than the contract: R and Y are rounded to bf16.)
TFLOP/s counts 2·M·N·K per candidate GEMM (4 formats + the reference).
--x-format bfp8 / bfp4 / bfp2: `fused` is the activation pre-pass (mtq_quantize_rows_bf16) plus one mtq_output_error_qx launch; the row
also reports the pre-pass alone (prepass_ms) and the W-only launch of the same session (w_only_ms), and qx_ratio = fused / W-only.
--layout transpose: `fused` is one mtq_output_error_transposed launch with the same candidates (bfp8 / bfp4 / bfp2 in the transposed
layout); the row also reports the row launch of the same session (rows_ms) and t_ratio = fused / rows.

  python tools/output_error_bench.py [--tokens 12800] [--reps 3] [--only mlp] [--x-format bfp8] [--layout transpose] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from quantization_analysis_amd import hip_backend as hb
from quantization_analysis_amd.model_source import TensorSpec, build_model_index

FMTS = ["bf16", "bfp8", "bfp4", "bfp2"]
MLP = {"model.layers.0.mlp.gate_proj.weight": (18432, 7168), "model.layers.0.mlp.up_proj.weight": (18432, 7168),
       "model.layers.0.mlp.down_proj.weight": (7168, 18432)}


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


def unfused(x, w):
    hi = w.to(torch.bfloat16)
    r = torch.matmul(x, hi.T).double()
    out = []
    for f in FMTS:
        wq = hb.quantize(w, f).to(torch.bfloat16)
        q = torch.matmul(x, wq.T).double()
        d = (r - q).abs()
        out.append(torch.stack([r.sum(), (r * r).sum(), q.sum(), (q * q).sum(), (r * q).sum(), d.sum(), d.max()]))
        del q, d
    return torch.stack(out)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=12800)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["all", "mlp"], default="all")
    ap.add_argument("--no-unfused", action="store_true")
    ap.add_argument("--x-format", choices=list(hb.X_FORMATS), default="bf16", help="the candidates' activation format (bf16: X as is)")
    ap.add_argument("--layout", choices=["rows", "transpose"], default="rows", help="the BFP layout of the fused launch")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    hb.require_gpu()
    dev = torch.device("cuda", 0)
    index = build_model_index("synthetic:deepseek-r1-layer0")
    for i, (name, shape) in enumerate(MLP.items()):
        index.specs[name] = TensorSpec(shape, "f32", 1000 + i, "fp8block")
    names = [n for n in index.tensor_names if len(index.specs[n].shape) == 2 and (args.only == "all" or n in MLP)]
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rows = []
    for name in names:
        w = index.load(name, device=dev, draw_on_device=True)
        n, k = w.shape
        x = torch.randn((args.tokens, k), generator=g, device=dev).to(torch.bfloat16)
        sums = torch.zeros((7, 7), dtype=torch.float64, device=dev)
        scratch = torch.empty((hb.output_error_scratch(args.tokens, n),), dtype=torch.float64, device=dev)
        mask = hb.fmt_mask(FMTS)

        oe = hb.output_error_transposed if args.layout == "transpose" else hb.output_error

        def fused():
            sums.zero_()
            oe(x, w, mask, sums, scratch=scratch)

        xq = torch.empty_like(x)

        def fused_qx():
            sums.zero_()
            oe(x, w, mask, sums, scratch=scratch, xq=hb.quantize_rows_bf16(x, args.x_format, out=xq))

        qx = args.x_format != "bf16"
        t_f = _time(fused_qx if qx else fused, args.reps)
        flop = 2.0 * args.tokens * n * k * (len(FMTS) + 1 + (1 if qx else 0))
        row = {"op": name, "N": n, "K": k, "M": args.tokens, "fused_ms": t_f * 1e3, "fused_tflops": flop / t_f / 1e12}
        if qx:
            t_p = _time(lambda: hb.quantize_rows_bf16(x, args.x_format, out=xq), max(args.reps, 10))
            t_w = _time(fused, args.reps)
            row.update({"x_format": args.x_format, "prepass_ms": t_p * 1e3, "w_only_ms": t_w * 1e3, "qx_ratio": t_f / t_w})
        if args.layout == "transpose":
            def rows_launch():
                sums.zero_()
                hb.output_error(x, w, mask, sums, scratch=scratch)

            t_r = _time(rows_launch, args.reps)
            row.update({"layout": "transpose", "rows_ms": t_r * 1e3, "t_ratio": t_f / t_r})
        if not args.no_unfused:
            t_u = _time(lambda: unfused(x, w), args.reps)
            row.update({"unfused_ms": t_u * 1e3, "unfused_tflops": flop / t_u / 1e12, "speedup": t_u / t_f})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del w, x, xq, scratch
        torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
