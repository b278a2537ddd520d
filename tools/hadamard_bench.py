"""mtq_hadamard_rows (csrc/mtq_hadamard.hip) on X of T × k, bf16 → bf16, with and without the bfp8 twin, against
  (a) what a user does without it: x.view(-1, B) @ H_B as a bf16 torch.matmul (H_B scaled by 2^(−p/2) and rounded to bf16: NOT the
      contract's bits — bf16 products accumulated by the GEMM, and for odd p a rounded scale);
  (b) torch.Tensor.copy_ of the same bytes: the bandwidth ceiling of one read and one write;
and one 7168 × 7168 float32 weight (the offline rotate_weight).  The kernel's output is compared with the float64 oracle on a slice
before any timing; then a warm-up and --reps event-timed regions per contender, alternating; medians.

    python tools/hadamard_bench.py [--reps 9] [--out profiles/hadamard.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from quantization_analysis_amd import hadamard as hd
from quantization_analysis_amd import hip_backend as hb


def timed(fns, reps: int, inner: int):
    """Median milliseconds per call of each fn: one warm-up round, then reps rounds that alternate between the contenders."""
    times = [[] for _ in fns]
    for r in range(reps + 1):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if r:
                times[i].append(a.elapsed_time(b) / inner)
    return [statistics.median(t) for t in times]


def case(T: int, k: int, block: int, dtype, reps: int):
    x = (torch.randn((T, k), device="cuda") * 3).to(dtype)
    y, yq, z = torch.empty_like(x), torch.empty((T, k), dtype=torch.bfloat16, device="cuda"), torch.empty_like(x)
    hb.hadamard_rows(x, block, out=y)
    rows = min(T, 4)
    want = hd.hadamard_emulation(x[:rows].cpu(), block, dtype)
    if dtype == torch.bfloat16:
        assert (y[:rows].cpu().float() - want.float()).abs().max() <= 2.0 ** -7 * want.float().abs().max(), "kernel output is off the oracle"
    else:
        assert torch.allclose(y[:rows].cpu(), want, rtol=1e-4, atol=1e-4 * float(want.abs().max())), "kernel output is off the oracle"
    h = torch.tensor([[1.0]])
    while h.shape[0] < block:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    hm = (h * float(hd.scale(block))).to(dtype).cuda()
    fns = [lambda: hb.hadamard_rows(x, block, out=y), lambda: torch.matmul(x.view(-1, block), hm, out=z.view(-1, block)), lambda: z.copy_(x)]
    if dtype == torch.bfloat16:
        fns.append(lambda: hb.hadamard_rows(x, block, out=y, q_fmt="bfp8", q_out=yq))
    inner = max(1, min(50, (1 << 27) // (T * k)))
    return timed(fns, reps, inner)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--out", default="profiles/hadamard.txt")
    args = p.parse_args(argv)
    torch.cuda.set_device(0)
    hb.require_gpu()
    lines = [f"mtq_hadamard_rows on {torch.cuda.get_device_name(0)}: medians of {args.reps} alternating event-timed regions after a warm-up, ms per call",
             "(a) bf16 torch.matmul with H_B (not the contract's bits); (b) copy_ of the same bytes; k/(a) and k/(b): kernel time over theirs",
             f"{'T':>6} {'k':>6} {'B':>5} {'dtype':>5} | {'kernel':>9} {'(a) gemm':>9} {'(b) copy':>9} | {'k/(a)':>6} {'k/(b)':>6} | {'+bfp8 twin':>10} {'twin/(b)':>8}"]
    cases = [(T, k, b, torch.bfloat16) for T in (1, 32, 4096, 16384) for k in (4096, 7168, 14336) for b in (32, hd.auto_block(k))]
    cases.append((7168, 7168, hd.auto_block(7168), torch.float32))
    for T, k, b, dtype in cases:
        t = case(T, k, b, dtype, args.reps)
        twin = f"{t[3]:10.4f} {t[3] / t[2]:8.2f}" if len(t) > 3 else f"{'-':>10} {'-':>8}"
        lines.append(f"{T:>6} {k:>6} {b:>5} {'bf16' if dtype == torch.bfloat16 else 'f32':>5} | {t[0]:9.4f} {t[1]:9.4f} {t[2]:9.4f} | "
                     f"{t[0] / t[1]:6.2f} {t[0] / t[2]:6.2f} | {twin}" + ("   <- loses to (a)" if t[0] > t[1] else ""))
        print(lines[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
