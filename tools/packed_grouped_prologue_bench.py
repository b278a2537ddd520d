"""The activation prologue of rotated / AWQ-scaled MoE experts on the decode route: inside the grouped skinny kernels (prologue="fused",
mtq_packed_glu_skinny_grouped_pre / mtq_packed_linear_skinny_grouped_pre) against the staged route (moe_dispatch, hadamard, a per-row
torch.ldexp, then the unfused grouped entry), by the method of DESIGN.md §A.6g: the outputs compared first, device events after a
warm-up, the sides alternated in one process, --rounds rounds of a window each, medians.

Rows: moe_glu (x (T, k) → h (S, hidden)) and moe_down_combine (h → y (T, k)) over --experts (count x hidden x k : topk), T in --tokens,
rotate in --blocks (0: none), with and without per-expert shifts, all-bfp4 maps, router ids uniform without repeats within a token:
  floor    the call without a prologue, the time the product alone takes;
  staged   prologue="staged"; timed TWICE per round (staged, staged2): the spread between the two medians is what a difference has to
           exceed to count;
  fused    prologue="fused".

  python tools/packed_grouped_prologue_bench.py [--rounds 5] [--window-ms 20] [--out profiles/packed_grouped_prologue.txt]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from quantization_analysis_amd import packed
from tools.packed_prologue_bench import time_sides


def experts(count: int, n: int, k: int, seed: int):
    """`count` packed (n, k) experts under all-bfp4 maps, generated and packed on the device in slabs of 32."""
    pts = []
    for e0 in range(0, count, 32):
        c = min(32, count - e0)
        w = torch.randn((c, n, k), generator=torch.Generator(device="cuda").manual_seed(seed + e0), device="cuda", dtype=torch.bfloat16)
        pts += packed.pack_batch(w, np.full((c, n // 32, k // 32), 2, dtype=np.int8), backend="hip")
    return packed.as_batch(pts)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=20.0)
    p.add_argument("--experts", default="256x2048x7168:8,8x4096x4096:2")
    p.add_argument("--tokens", default="1,8,32")
    p.add_argument("--blocks", default="0,256")
    p.add_argument("--out", default="profiles/packed_grouped_prologue.txt")
    a = p.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    lines = [f"# tools/packed_grouped_prologue_bench.py --rounds {a.rounds} --window-ms {a.window_ms}: medians in us per call; all-bfp4 maps; "
             "kernel='walk', split 0 on every side (the fused rule may choose a smaller split than the unfused one)",
             f"{'stage':>16} {'experts':>16} {'T':>3} {'block':>5} {'shifts':>6} {'floor':>8} {'staged':>8} {'staged2':>8} {'fused':>8} "
             f"{'fused/staged':>12} {'spread':>7}"]
    for spec in a.experts.split(","):
        shape, topk = spec.split(":")
        count, hidden, k = (int(v) for v in shape.split("x"))
        topk = int(topk)
        gate, up, down = experts(count, hidden, k, 1), experts(count, hidden, k, 2), experts(count, k, hidden, 3)
        for T in (int(t) for t in a.tokens.split(",")):
            ids = torch.from_numpy(np.stack([rng.choice(count, topk, replace=False) for _ in range(T)])).cuda()
            plan = packed.moe_plan(ids, count)
            w = torch.rand((T, topk), device="cuda")
            x = torch.randn((T, k), device="cuda").to(torch.bfloat16)
            h = torch.randn((T * topk, hidden), device="cuda").to(torch.bfloat16)
            stages = (("moe_glu", k, lambda **kw: packed.moe_glu(x, plan, gate, up, **kw)),
                      ("moe_down_combine", hidden, lambda **kw: packed.moe_down_combine(h, w, plan, down, out_dtype="bfloat16", **kw)))
            for stage, width, call in stages:
                for B in (int(b) for b in a.blocks.split(",")):
                    for shifts in (None, packed._GroupShifts(rng.integers(0, 8, (count, width)), count, width, "cuda")):
                        if not B and shifts is None:
                            continue
                        kw = dict(rotate=B, in_exponents=shifts)
                        got, want = call(prologue="fused", **kw).float(), call(prologue="staged", **kw).float()
                        err = float((got - want).abs().max() / want.abs().max())      # equal splits give equal bits; the rules may differ
                        assert err < 2e-2, (stage, spec, T, B, err)
                        sides = [{"name": "floor", "fn": lambda i: call()}, {"name": "staged", "fn": lambda i: call(prologue="staged", **kw)},
                                 {"name": "staged2", "fn": lambda i: call(prologue="staged", **kw)},
                                 {"name": "fused", "fn": lambda i: call(prologue="fused", **kw)}]
                        time_sides(sides, a.rounds, a.window_ms)
                        t = {s["name"]: s["med"] for s in sides}
                        lines.append(f"{stage:>16} {shape:>16} {T:>3} {B:>5} {'yes' if shifts is not None else 'no':>6} {t['floor']:>8.1f} "
                                     f"{t['staged']:>8.1f} {t['staged2']:>8.1f} {t['fused']:>8.1f} "
                                     f"{t['fused'] / min(t['staged'], t['staged2']):>12.3f} {abs(t['staged'] - t['staged2']):>7.2f}")
                        print(lines[-1], flush=True)
        del gate, up, down
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
