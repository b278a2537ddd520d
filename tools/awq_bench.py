"""mtq_awq_losses (csrc/mtq_awq.hip): the AWQ search over G′ = 20 shift rows against what a user has without it: per row, ldexp → hb.quantize → ldexp, then one LOE pass with X·Ŵᵀ (a float32 torch GEMM) as the recorded output,
the loss read from the sums as Σr² − 2Σrq + Σq².  bfp4 codes, M synthetic N(0, 1) bf16 tokens with every 64th channel 32× its
neighbours, W ~ 0.02·t₃ as bf16 and as float32, on an MLP and an attention shape of synthetic:deepseek-r1-layer0.  The two loss
vectors are compared before any timing; then a warm-up and --reps event-timed regions per contender, alternating; medians.
TFLOP/s is the useful rate, 2·M·N·K·(20 + 1) per search: R counted once, although every launch of 5 slots forms it again (and in three
passes, hi / mid / lo, for float32 W).

    python tools/awq_bench.py [--reps 5] [--tokens 4096] [--out profiles/awq_search.txt]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import awq, hip_backend as hb
from quantization_analysis_amd.gptq import constant_codes
from tools.hadamard_bench import timed

SHAPES = {"mlp.down_proj": (7168, 18432), "mlp.gate_proj": (18432, 7168), "self_attn.o_proj": (7168, 16384)}


def case(name, n, k, m, dtype, reps):
    g = torch.Generator(device="cuda").manual_seed(n + k)
    x = torch.randn((m, k), device="cuda", generator=g)
    x[:, ::64] *= 32.0
    x = x.to(torch.bfloat16)
    chi = torch.randn((3, n, k), device="cuda", generator=g).pow(2).sum(0)
    w = (torch.randn((n, k), device="cuda", generator=g) / (chi / 3.0).sqrt() * 0.02).to(dtype)    # 0.02·t₃
    del chi
    codes = constant_codes(n, k, "bfp4")
    t = np.log2(x.float().pow(2).mean(0).sqrt().cpu().numpy().astype(np.float64))
    _alphas, p = awq.exponent_table(t, 20, 7)
    while p.shape[0] < 20:                                               # G′ = 20 exactly: duplicates dropped by the table are put back
        p = np.concatenate([p, p[-1:]])
    cd, pd = torch.from_numpy(codes).cuda(), torch.from_numpy(p).cuda()
    scratch = torch.empty((hb.awq_losses_scratch(m, n, 20),), dtype=torch.float64, device="cuda")
    oe_scratch = torch.empty((hb.output_error_scratch(m, n),), dtype=torch.float64, device="cuda")
    loss = torch.zeros((20,), dtype=torch.float64, device="cuda")

    def fused():
        loss.zero_()
        hb.awq_losses(x, w, cd, pd, loss, scratch, checked=True)
        return loss

    base_loss = torch.zeros((20,), dtype=torch.float64, device="cuda")

    def baseline():
        wf = w.float()
        for i in range(20):
            e = pd[i].to(torch.int32)
            what = torch.ldexp(hb.quantize(torch.ldexp(wf, e), "bfp4"), -e)
            sums = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
            hb.output_error(x, w, 0, sums, recorded=x.float() @ what.T, scratch=oe_scratch)
            s = sums[6]
            base_loss[i] = s[1] - 2.0 * s[4] + s[3]
        return base_loss

    hb.awq_check_values(w, cd, pd)
    got, base = fused().clone(), baseline().clone()
    assert torch.allclose(got, base, rtol=1e-3), (got, base)
    tf, tb = timed([fused, baseline], reps, 1)
    best = int(got.argmin())
    return (f"{name:>16} {n:>6} {k:>6} {m:>6} {'f32' if dtype == torch.float32 else 'bf16':>5} | {tf:9.2f} {tb:9.2f} | {tb / tf:6.2f} | "
            f"{2.0 * m * n * k * 21 / tf / 1e9:7.1f} | g* {best:2d} loss {float(got[best]):.6e} rtn {float(got[0]):.6e}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--out", default="profiles/awq_search.txt")
    args = ap.parse_args(argv)
    torch.cuda.set_device(0)
    hb.require_gpu()
    lines = [f"mtq_awq_losses, G' = 20, bfp4, on {torch.cuda.get_device_name(0)}: medians of {args.reps} alternating event-timed regions after a warm-up, ms per search",
             "baseline = 20 x (ldexp, hb.quantize, ldexp, float32 GEMM X·Ŵᵀ, mtq_output_error with it as recorded); TF/s = 2·M·N·K·21 / fused time",
             f"{'op':>16} {'N':>6} {'K':>6} {'M':>6} {'W':>5} | {'fused':>9} {'baseline':>9} | {'base/f':>6} | {'TF/s':>7} | losses"]
    for name, (n, k) in SHAPES.items():
        for dtype in (torch.bfloat16, torch.float32):
            lines.append(case(name, n, k, args.tokens, dtype, args.reps))
            print(lines[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
